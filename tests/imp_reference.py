"""IMP restated (torch, CPU): what imcui/hloc/matchers/imp.py:40-51 runs -- `pram.nets.gml.GML(conf)`, a strict `load_state_dict`
and `produce_matches(data, p=0.2)`.  TEST INFRASTRUCTURE ONLY.

The reference checkout ships no `imcui/third_party/pram`, so the network is restated from its description: parity unpinned
("IMP: what is pinned", lists what rests on memory).  `GML` is an nn.Module whose state-dict names and shapes are the
table of csrc/imp.hip; `.double()` gives the float64 oracle.  tests/golden/make_imp_golden.py injects this module as `pram.nets.gml`
into the reference's own wrapper.

  * key-points normalised by (k - [W, H] / 2) / (0.7 max(W, H)); `kenc.encoder` = Conv1d 3-32-64-128-256-256 on [x, y, score]
    with BatchNorm1d + ReLU after every layer but the last; desc = input_proj(desc) + kenc(kpts, scores);
  * 18 attentional propagation layers ['self', 'cross'] * 9 (SuperGlue's: heads interleaved, view(B, 64, 4, N));
  * final_proj.{0..8}, inference reads .8; M = md0 . md1 / 256 ** .5; a dust-bin column, then a dust-bin row of `bin_score`;
  * probability-domain Sinkhorn (`sinkhorn`), then mutual arg-max with the strict threshold p (`matches_from_assignment`).

Intended divergence: equal maxima go to the LOWEST index (`first_argmax`); torch.max leaves that open.

`sinkhorn_explicit` is the assignment stage in the float32 operation order of the imp_* kernels (numpy, every operation rounds once).
"""
from __future__ import annotations

import numpy as np
import torch
from torch import nn

EPS = 1e-8
DEFAULT_CONF = {
    "descriptor_dim": 128,
    "hidden_dim": 256,
    "keypoint_encoder": [32, 64, 128, 256],
    "GNN_layers": ["self", "cross"] * 9,
    "n_layers": 9,
    "n_heads": 4,
    "sinkhorn_iterations": 20,
    "with_sinkhorn": True,
    "ac_fn": "relu",
    "norm_fn": "bn",
    "match_threshold": 0.2,
}


def mlp(channels: list) -> nn.Sequential:
    layers = []
    for i in range(1, len(channels)):
        layers.append(nn.Conv1d(channels[i - 1], channels[i], kernel_size=1, bias=True))
        if i < len(channels) - 1:
            layers += [nn.BatchNorm1d(channels[i]), nn.ReLU()]
    return nn.Sequential(*layers)


def normalize_keypoints(kpts: torch.Tensor, image_shape) -> torch.Tensor:
    _, _, height, width = image_shape
    size = kpts.new_tensor([[float(width), float(height)]])
    center = size / 2
    scaling = size.max(1, keepdim=True).values * 0.7
    return (kpts - center[:, None, :]) / scaling[:, None, :]


class KeypointEncoder(nn.Module):
    def __init__(self, feature_dim, layers):
        super().__init__()
        self.encoder = mlp([3] + list(layers) + [feature_dim])

    def forward(self, kpts, scores):
        return self.encoder(torch.cat([kpts.transpose(1, 2), scores.unsqueeze(1)], dim=1))


class MultiHeadedAttention(nn.Module):
    def __init__(self, heads, d):
        super().__init__()
        self.dim, self.heads = d // heads, heads
        self.merge = nn.Conv1d(d, d, kernel_size=1)
        self.proj = nn.ModuleList([nn.Conv1d(d, d, kernel_size=1) for _ in range(3)])

    def forward(self, q, k, v):
        b = q.shape[0]
        q, k, v = (l(x).view(b, self.dim, self.heads, -1) for l, x in zip(self.proj, (q, k, v)))
        prob = torch.softmax(torch.einsum("bdhn,bdhm->bhnm", q, k) / self.dim**0.5, dim=-1)
        x = torch.einsum("bhnm,bdhm->bdhn", prob, v)
        return self.merge(x.contiguous().view(b, self.dim * self.heads, -1))


class AttentionalPropagation(nn.Module):
    def __init__(self, d, heads):
        super().__init__()
        self.attn = MultiHeadedAttention(heads, d)
        self.mlp = mlp([2 * d, 2 * d, d])

    def forward(self, x, source):
        return self.mlp(torch.cat([x, self.attn(x, source, source)], dim=1))


class AttentionalGNN(nn.Module):
    def __init__(self, d, names, heads):
        super().__init__()
        self.layers = nn.ModuleList([AttentionalPropagation(d, heads) for _ in names])
        self.names = list(names)

    def forward(self, desc0, desc1):
        for layer, name in zip(self.layers, self.names):
            src0, src1 = (desc1, desc0) if name == "cross" else (desc0, desc1)
            delta0, delta1 = layer(desc0, src0), layer(desc1, src1)
            desc0, desc1 = desc0 + delta0, desc1 + delta1
        return desc0, desc1


def first_argmax(x: torch.Tensor, dim: int):
    """(values, indices) of the maximum along `dim`, equal maxima to the lowest index."""
    vals = x.max(dim, keepdim=True).values
    shape = [1] * x.dim()
    shape[dim] = -1
    ar = torch.arange(x.shape[dim], device=x.device).view(shape).expand_as(x)
    idx = torch.where(x == vals, ar, torch.full_like(ar, x.shape[dim])).min(dim).values
    return vals.squeeze(dim), idx


def augment(scores: torch.Tensor, bin_score) -> torch.Tensor:
    """[B, n, m] -> [B, n + 1, m + 1]: a column, then a row of bin_score (corner included)."""
    b, n, m = scores.shape
    alpha = torch.as_tensor(bin_score, dtype=scores.dtype).to(scores.device)
    M = torch.cat([scores, alpha.expand(b, n, 1)], dim=-1)
    return torch.cat([M, alpha.expand(b, 1, m + 1)], dim=-2)


def sinkhorn(M: torch.Tensor, iters: int, eps: float = EPS):
    """Probability-domain Sinkhorn on the augmented scores [B, n + 1, m + 1]: (P, u, v).  r = [1] * n + [m], c = [1] * m + [n]."""
    b, n1, m1 = M.shape
    n, m = n1 - 1, m1 - 1
    p = torch.softmax(M, dim=-1)
    r = torch.cat([M.new_ones(n), M.new_tensor([float(m)])])[None].expand(b, -1)
    c = torch.cat([M.new_ones(m), M.new_tensor([float(n)])])[None].expand(b, -1)
    u, v = torch.ones_like(r), torch.ones_like(c)
    for _ in range(iters):
        u = r / ((p * v[:, None, :]).sum(-1) + eps)
        v = c / ((p * u[:, :, None]).sum(-2) + eps)
    return p * u[:, :, None] * v[:, None, :], u, v


def matches_from_assignment(P: torch.Tensor, p: float) -> dict:
    """P [B, n + 1, m + 1] -> the output dictionary of produce_matches (strict threshold, scores are probabilities)."""
    inner = P[:, :-1, :-1]
    max0, indices0 = first_argmax(inner, 2)
    _, indices1 = first_argmax(inner, 1)
    ar0 = torch.arange(indices0.shape[1], device=P.device)[None]
    ar1 = torch.arange(indices1.shape[1], device=P.device)[None]
    mutual0 = ar0 == indices1.gather(1, indices0)
    mutual1 = ar1 == indices0.gather(1, indices1)
    zero = P.new_tensor(0)
    mscores0 = torch.where(mutual0, max0, zero)
    mscores1 = torch.where(mutual1, mscores0.gather(1, indices1), zero)
    valid0 = mutual0 & (mscores0 > P.new_tensor(p))  # the scalar takes the tensor's dtype, as `tensor > 0.2` does
    valid1 = mutual1 & valid0.gather(1, indices1)
    return {
        "matches0": torch.where(valid0, indices0, indices0.new_tensor(-1)),
        "matches1": torch.where(valid1, indices1, indices1.new_tensor(-1)),
        "matching_scores0": mscores0,
        "matching_scores1": mscores1,
    }


SCORE_BAR = 1e-4  # the project's bar for matcher scores (tests/test_gpu_superglue.py)


def decision_margin(P: torch.Tensor, p: float, floor: float = SCORE_BAR) -> float:
    """Of one pair's float64 P [n + 1, m + 1]: the smallest of the rows' top-2 gaps, the columns' top-2 gaps and |mscore - p| over the
    mutual candidates, on the real rows and columns.

    The gaps are taken over the rows and columns whose largest entry reaches `floor`, the bar of the score comparison.  A row or column
    below it cannot move a compared output past its bar, whichever way its arg-max falls: a match needs P_ij > p, so both its row and its
    column hold an entry above p, and a score that appears or vanishes with a flipped mutual flag is that row's maximum, below the bar.
    Without the restriction no problem with outliers has a margin: the entries of an unmatched row are of the order of 1e-15 and so are
    their gaps.  A row whose maximum lies between `floor` and the demanded margin fails it by construction (gap <= maximum)."""
    inner = P[:-1, :-1].detach().double()
    n, m = inner.shape
    gaps = []
    for dim, k in ((1, m), (0, n)):
        if k > 1:
            t = inner.topk(2, dim=dim).values
            top, second = (t[:, 0], t[:, 1]) if dim == 1 else (t[0], t[1])
            live = top >= floor
            if live.any():
                gaps.append(float((top - second)[live].min()))
    max0, i0 = first_argmax(inner[None], 2)
    mutual = first_argmax(inner[None], 1)[1][0][i0[0]] == torch.arange(n)
    if mutual.any():
        gaps.append(float((max0[0][mutual] - p).abs().min()))
    return min(gaps) if gaps else float("inf")


def assign(scores: torch.Tensor, bin_score, iters: int, p: float = 0.2) -> dict:
    """The assignment stage alone on scores [B, n, m] (any float dtype): matches, scores, u, v and P."""
    P, u, v = sinkhorn(augment(scores, bin_score), iters)
    return {**matches_from_assignment(P, p), "u": u, "v": v, "P": P}


class GML(nn.Module):
    default_config = DEFAULT_CONF

    def __init__(self, config: dict | None = None):
        super().__init__()
        self.config = {**self.default_config, **(config or {})}
        c = self.config
        if c["n_layers"] != 9 or not c["with_sinkhorn"]:
            raise ValueError("restated for n_layers = 9 with the Sinkhorn assignment only")
        d = c["hidden_dim"]
        self.sinkhorn_iterations = c["sinkhorn_iterations"]
        self.kenc = KeypointEncoder(d, c["keypoint_encoder"])
        self.input_proj = nn.Conv1d(c["descriptor_dim"], d, kernel_size=1, bias=True)
        self.gnn = AttentionalGNN(d, c["GNN_layers"], c["n_heads"])
        self.final_proj = nn.ModuleList([nn.Conv1d(d, d, kernel_size=1, bias=True) for _ in range(c["n_layers"])])
        self.bin_score = nn.Parameter(torch.tensor(1.0))

    def scores(self, data: dict) -> torch.Tensor:
        dt = self.bin_score.dtype
        desc0, desc1 = data["descriptors0"].to(dt).transpose(1, 2), data["descriptors1"].to(dt).transpose(1, 2)  # [B, N, 128] in
        kpts0 = normalize_keypoints(data["keypoints0"].to(dt), data["image0"].shape)
        kpts1 = normalize_keypoints(data["keypoints1"].to(dt), data["image1"].shape)
        desc0 = self.input_proj(desc0) + self.kenc(kpts0, data["scores0"].to(dt))
        desc1 = self.input_proj(desc1) + self.kenc(kpts1, data["scores1"].to(dt))
        desc0, desc1 = self.gnn(desc0, desc1)
        md0, md1 = self.final_proj[-1](desc0), self.final_proj[-1](desc1)
        return torch.einsum("bdn,bdm->bnm", md0, md1) / self.config["hidden_dim"] ** 0.5

    @torch.no_grad()
    def produce_matches(self, data: dict, p: float = 0.2, full: bool = False) -> dict:
        out = assign(self.scores(data), self.bin_score.detach(), self.sinkhorn_iterations, p)
        return out if full else {k: out[k] for k in ("matches0", "matches1", "matching_scores0", "matching_scores1")}


def problem(seed: int, n: int, m: int, n_out: int, noise: float = 0.05, size=(640, 480)) -> dict:
    """Key-points, scores and distinctive 128-d unit descriptors with known correspondences, as the [B = 1] dictionary `produce_matches`
    takes (descriptors [1, N, 128]); "partner" [m]: the point of image 0 behind point j of image 1, -1 for the last `n_out` (outliers)."""
    import torch.nn.functional as Fn

    g = torch.Generator().manual_seed(seed)
    W, H = size
    box = torch.tensor([W - 8.0, H - 8.0])
    k0 = torch.rand(n, 2, generator=g) * box + 4
    perm = torch.randperm(n, generator=g)[torch.arange(m) % n]  # m > n: the extra points re-use partners and become outliers
    k1 = k0[perm] + torch.randn(m, 2, generator=g)
    d0 = Fn.normalize(torch.randn(n, 128, generator=g), dim=1)
    d1 = Fn.normalize(d0[perm] + noise * torch.randn(m, 128, generator=g), dim=1)
    n_out = max(n_out, m - n)
    if n_out:
        d1[m - n_out :] = Fn.normalize(torch.randn(n_out, 128, generator=g), dim=1)
        k1[m - n_out :] = torch.rand(n_out, 2, generator=g) * box + 4
    partner = perm.clone()
    partner[m - n_out :] = -1
    img0 = torch.zeros(1, 1, H, W)
    return {"image0": img0, "image1": img0, "keypoints0": k0[None], "keypoints1": k1[None], "scores0": torch.rand(1, n, generator=g),
            "scores1": torch.rand(1, m, generator=g), "descriptors0": d0[None], "descriptors1": d1[None], "partner": partner}  # fmt: skip


MIN_MARGIN = 1e-3  # ten times the score bar
MAX_SEEDS = 40


def search_problem(net64: "GML", seed0: int, n: int, m: int, n_out: int, iters: tuple, p: float = 0.2, size=(640, 480)):
    """The first seed >= seed0 (at most MAX_SEEDS tried) whose float64 decision margin is at least MIN_MARGIN at every round count of
    `iters`: (data, {rounds: float64 result with "P" and "margin"}).  The network runs once per seed, the assignment once per count."""
    for seed in range(seed0, seed0 + MAX_SEEDS):
        data = problem(seed, n, m, n_out, size=size)
        with torch.no_grad():
            sc = net64.scores(data)
        ref = {}
        for it in iters:
            r = assign(sc, net64.bin_score.detach(), it, p)
            r["margin"] = decision_margin(r["P"][0], p)
            ref[it] = r
        if min(r["margin"] for r in ref.values()) >= MIN_MARGIN:
            data["seed"] = seed
            return data, ref
    raise AssertionError(f"no seed in {seed0}..{seed0 + MAX_SEEDS - 1} reaches a decision margin of {MIN_MARGIN} at {n} x {m}")


def oracle(state_dict: dict, iters: int, double: bool = True) -> GML:
    net = GML({"sinkhorn_iterations": iters}).eval()
    net.load_state_dict(state_dict, strict=True)
    return net.double() if double else net


# ------------------------------------------------------------------ the assignment stage in the kernels' float32 order
F = np.float32


def _lane_sums(x: np.ndarray) -> np.ndarray:
    """x [rows, cols] float32 -> [rows]: a lane owns columns k * 256 + 4 * lane + c and adds them k-major, c-minor; the 64 lanes fold as a
    tree (l with l ^ 32, then ^ 16, ... ^ 1).  imp_softmax_kernel / imp_round_kernel."""
    rows, cols = x.shape
    nk = -(-cols // 256)
    pad = np.zeros((rows, nk * 256), F)
    pad[:, :cols] = x
    t = pad.reshape(rows, nk, 64, 4)
    s = np.zeros((rows, 64), F)
    for k in range(nk):
        for c in range(4):
            s = s + t[:, k, :, c]
    return _tree(s)


def _tree(s: np.ndarray) -> np.ndarray:
    o = s.shape[-1] // 2
    while o >= 1:
        s = s[..., :o] + s[..., o : 2 * o]
        o //= 2
    return s[..., 0]


def _strided_sum(x: np.ndarray, threads: int) -> np.float32:
    """thread t adds x[t], x[t + threads], ...; waves of 64 threads fold as a tree; the waves are added in order."""
    n = -(-len(x) // threads)
    pad = np.zeros(n * threads, F)
    pad[: len(x)] = x
    s = np.zeros(threads, F)
    for r in pad.reshape(n, threads):
        s = s + r
    waves = _tree(s.reshape(threads // 64, 64))
    S = waves[0]
    for w in waves[1:]:
        S = S + w
    return S


def sinkhorn_explicit(scores: np.ndarray, bin_score: float, iters: int):
    """One pair, scores [n, m] float32 -> (p [n, m], binc [n], u [n + 1], v [m + 1]) in the order of csrc/imp.hip; the assignment is
    (p_ij u_i) v_j."""
    z = np.asarray(scores, F)
    n, m = z.shape
    alpha, eps, one = F(bin_score), F(EPS), F(1)
    mx = np.maximum(z.max(1), alpha)
    e = np.exp(z - mx[:, None], dtype=F)
    eb = np.exp(alpha - mx, dtype=F)
    tot = _lane_sums(e) + eb
    p, binc = e / tot[:, None], eb / tot
    u, v = np.ones(n + 1, F), np.ones(m + 1, F)
    dbrow = one / F(m + 1)
    nb = -(-n // 16)
    for _ in range(iters):
        u[:n] = one / ((_lane_sums(p * v[None, :m]) + binc * v[m]) + eps)
        u[n] = F(m) / (_strided_sum(dbrow * v, 512) + eps)
        pu = np.zeros((nb * 16, m), F)
        pu[:n] = p * u[:n, None]
        pu = pu.reshape(nb, 8, 2, m)
        wave = pu[:, :, 0] + pu[:, :, 1]  # a wave's two rows
        part = wave[:, 0]
        for w in range(1, 8):
            part = part + wave[:, w]  # the band: waves in order
        groups = []
        for g in range(0, nb, 16):
            t = np.zeros(m, F)
            for k in range(g, min(nb, g + 16)):
                t = t + part[k]
            groups.append(t)
        r = groups[0]
        for t in groups[1:]:
            r = r + t
        rowterm = dbrow * u[n]
        v[:m] = one / ((r + rowterm) + eps)
        v[m] = F(n) / ((_strided_sum(binc * u[:n], 1024) + rowterm) + eps)
    return p, binc, u, v


def assign_explicit(scores: np.ndarray, bin_score: float, iters: int, p: float = 0.2) -> dict:
    pr, _, u, v = sinkhorn_explicit(scores, bin_score, iters)
    n, m = pr.shape
    P = torch.zeros(1, n + 1, m + 1)
    P[0, :n, :m] = torch.from_numpy((pr * u[:n, None]) * v[None, :m])
    return {**matches_from_assignment(P, p), "u": torch.from_numpy(u)[None], "v": torch.from_numpy(v)[None]}


# ------------------------------------------------------------------ score matrices for the assignment stage alone
RANDOM_BIN = 12.0  # dust-bin score of the random matrices below


def random_scores(seed: int, n: int, m: int) -> torch.Tensor:
    """[n, m] float32: N(0, 0.5^2) noise, a planted partial permutation at +24, and for an eighth of it a rival row at +23 on the same
    column, so that the rounds have mass to move (a column claimed twice starts at a sum near 2) while every decision stays clear."""
    g = torch.Generator().manual_seed(seed)
    z = 0.5 * torch.randn(n, m, generator=g)
    k = min(n, m)
    rows, cols = torch.randperm(n, generator=g)[:k], torch.randperm(m, generator=g)[:k]
    z[rows, cols] += 24.0
    for t in range(k // 8):
        a = int(torch.randint(0, n, (1,), generator=g))
        if a != int(rows[t]):
            z[a, cols[t]] += 23.0
    return z


def search_scores(seed0: int, n: int, m: int, iters: tuple, bin_score: float = RANDOM_BIN, p: float = 0.2):
    """The first seed >= seed0 (at most MAX_SEEDS) whose float64 decision margin reaches MIN_MARGIN at every round count: (scores [n, m]
    float32, {rounds: float64 result with "margin"})."""
    for seed in range(seed0, seed0 + MAX_SEEDS):
        z = random_scores(seed, n, m)
        ref = {}
        for it in iters:
            r = assign(z[None].double(), bin_score, it, p)
            r["margin"] = decision_margin(r["P"][0], p)
            ref[it] = r
        if min(r["margin"] for r in ref.values()) >= MIN_MARGIN:
            return z, ref
    raise AssertionError(f"no seed in {seed0}..{seed0 + MAX_SEEDS - 1} reaches a decision margin of {MIN_MARGIN} at {n} x {m}")


def crafted_cases() -> dict:
    """name -> (scores [n, m] float32, bin_score, rounds, p, expected matches0 or None): the crafted matrices of the assignment tests.
    `expected` is what the construction demands; tests/test_imp_cpu.py holds the float64 restatement to it."""
    g = torch.Generator().manual_seed(123)
    cases = {}
    # every entry equal: all rows and all columns tie, ties go to the lowest index, so (0, 0) is the only mutual pair
    cases["constant"] = (torch.full((5, 7), 0.5), 0.5, 3, 0.01, [0, -1, -1, -1, -1])
    # +-80: exp(-160) is 0 in float32; without the maximum subtracted exp(80) overflows.  Row 5 ties with row 2 on column 4 (lowest wins)
    z = torch.full((6, 9), -80.0)
    perm = [3, 0, 4, 8, 1, 4]
    for i, j in enumerate(perm):
        z[i, j] = 80.0
    cases["pm80"] = (z, 0.0, 5, 0.2, [3, 0, 4, 8, 1, -1])
    # a dust-bin score far above every real score: all mass goes to the dust-bins, nothing passes p
    cases["bin_dominates"] = (torch.randn(9, 6, generator=g), 30.0, 20, 0.2, [-1] * 9)
    # a dust-bin score of -30: the dust-bins start empty, the planted permutation is found
    z = torch.randn(8, 8, generator=g)
    perm = torch.randperm(8, generator=g)
    z[torch.arange(8), perm] += 12.0
    cases["bin_minus30"] = (z, -30.0, 20, 0.2, perm.tolist())
    # row 2: real entries 200 below the dust-bin, exp underflows in float32 (not in float64): p_2j = 0, the division is held by eps
    # and the dust-bin entry; the row stays unmatched and its neighbours keep their planted partners
    z = torch.randn(6, 6, generator=g)
    z[torch.arange(6), torch.arange(6)] += 15.0
    z[2] = -200.0
    cases["underflow_row"] = (z, 0.0, 20, 0.2, [0, 1, -1, 3, 4, 5])
    return cases
