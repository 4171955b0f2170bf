"""Plain-torch restatement of the DeDoDe extractor as imcui/hloc/extractors/dedode.py:55-86 runs it (Parskatt/DeDoDe:
dedode_detector_L.detect, dedode_descriptor_B.describe_keypoints, utils.sample_keypoints / get_grid / to_pixel_coords), CPU, float32 or
float64.

Upstream's package is not vendored: the networks are restated from their description and their parity with upstream's code is not
pinned ("DeDoDe: what is pinned").  The wrapper -- Normalize, the order of the two models, the output layouts -- is read
from the reference and restated literally.  Layer shapes are read from the state dicts, never hard-coded.

The detection arithmetic exists in two forms.  `scores_library` is upstream's: softmax, F.conv2d with the 51 taps, `** -0.5`.
`scores_explicit` is ONE written-out float32 order, the one csrc/dedode.hip uses, in which every torch op rounds once:
    log p = (l - max) - log(sum exp(l - max));  p = exp_explicit(log p)  (Cephes expf: n = round(x log2 e), r = (x - n C1) - n C2, a
    degree-5 Horner polynomial, 2^n by ldexp; arguments clamped at -80);  q = (p + 1e-6) * 10000;  the taps w[0..50] summed in ascending
    order along the row, then along the column, zero padding;  score = p * (1 / sqrt(density + 1e-8)), root and quotient correctly rounded
The key-point of pixel (i, j) is x = (2 j + 1) / W - 1 (get_grid's pixel centre), to_pixel_coords = ((x + 1) / 2) W.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

ENCODERS = {"detector": (64, 64, "M", 128, 128, "M", 256, 256, 256, 256, "M", 512, 512, 512, 512, "M"),
            "descriptor": (64, "M", 128, "M", 256, 256, "M", 512, 512, "M")}  # fmt: skip
SCALES = (8, 4, 2, 1)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
DEFAULT_CONF = {"name": "dedode", "model_detector_name": "dedode_detector_L.pth", "model_descriptor_name": "dedode_descriptor_B.pth",
                "max_keypoints": 2000, "match_threshold": 0.2, "dense": False}  # fmt: skip
NTAPS = 51


def _bn(sd, p, x):
    return F.batch_norm(x, sd[p + ".running_mean"].to(x), sd[p + ".running_var"].to(x), sd[p + ".weight"].to(x), sd[p + ".bias"].to(x), False, 0.0, 1e-5)


def encoder(sd: dict, x: torch.Tensor, model: str) -> list:
    """x [B,3,H,W] normalised -> the maps in front of the four max-pools, scales 1, 2, 4, 8."""
    feats, op = [], 0
    for v in ENCODERS[model]:
        if v == "M":
            feats.append(x)
            x = F.max_pool2d(x, 2, 2)
            op += 1
        else:
            p = f"encoder.layers.{op}"
            x = F.relu(_bn(sd, f"encoder.layers.{op + 1}", F.conv2d(x, sd[p + ".weight"].to(x), sd[p + ".bias"].to(x), padding=1)))
            op += 3
    return feats


def _block(sd, p, x):
    """create_block: conv (1x1, or depth-wise 5x5 when the weight says so), BatchNorm, ReLU, conv1x1."""
    w = sd[p + ".0.weight"].to(x)
    depthwise = w.shape[1] == 1 and w.shape[-1] > 1
    x = F.conv2d(x, w, sd[p + ".0.bias"].to(x), padding=w.shape[-1] // 2, groups=w.shape[0] if depthwise else 1)
    x = F.relu(_bn(sd, p + ".1", x))
    return F.conv2d(x, sd[p + ".3.weight"].to(x), sd[p + ".3.bias"].to(x))


def refiner_hidden(sd: dict, p: str, x: torch.Tensor) -> torch.Tensor:
    """ConvRefiner up to `(hidden_blocks(x0) + x0) / 1.4`."""
    x0 = _block(sd, p + ".block1", x)
    y, i = x0, 0
    while f"{p}.hidden_blocks.{i}.0.weight" in sd:
        y = _block(sd, f"{p}.hidden_blocks.{i}", y)
        i += 1
    return (y + x0) / 1.4


def refiner(sd: dict, p: str, x: torch.Tensor) -> torch.Tensor:
    return F.conv2d(refiner_hidden(sd, p, x), sd[p + ".out_conv.weight"].to(x), sd[p + ".out_conv.bias"].to(x))


def decode(sd: dict, img: torch.Tensor, model: str) -> list:
    """-> the accumulated logits of the scales 8, 4, 2, 1 ([B,P,h,w] each; P = 1 key-point logit / 256 description channels)."""
    P = 1 if model == "detector" else 256
    mode = "bicubic" if model == "detector" else "bilinear"
    feats = encoder(sd, img, model)[::-1]
    acc, ctx, accs = None, None, []
    for i, (s, f) in enumerate(zip(SCALES, feats)):
        o = refiner(sd, f"decoder.layers.{s}", f if ctx is None else torch.cat([f, ctx], 1))
        acc = o[:, :P] if acc is None else acc + o[:, :P]
        accs.append(acc)
        if s != 1:
            size = feats[i + 1].shape[2:]
            acc = F.interpolate(acc, size=size, mode=mode, align_corners=False)
            ctx = F.interpolate(o[:, P:], size=size, mode="bilinear", align_corners=False)
    return accs


def density_taps(dtype=torch.float32, device="cpu") -> torch.Tensor:
    return torch.exp(-torch.linspace(-2, 2, NTAPS, dtype=torch.float32) ** 2).to(device=device, dtype=dtype)


def exp_explicit(x: torch.Tensor) -> torch.Tensor:
    """Cephes expf in single torch ops (float32 in, every op rounds once): the bits of csrc/dedode.hip's dd_exp."""
    x = torch.clamp(x, min=-80.0)
    n = torch.round(x * 1.44269504088896341)
    r = (x - n * 0.693359375) - n * (-2.12194440e-4)
    p = torch.full_like(x, 1.9875691500e-4)
    for c in (1.3981999507e-3, 8.3334519073e-3, 4.1665795894e-2, 1.6666665459e-1, 5.0000001201e-1):
        p = p * r + c
    y = (p * (r * r) + r) + 1.0
    if x.dtype != torch.float32:
        return torch.ldexp(y, n.to(torch.int32))
    return y * ((n.to(torch.int32) + 127) << 23).view(torch.float32)  # 2^n exactly, from its bits (n >= -116: a normal number)


def filter_explicit(v: torch.Tensor, w: torch.Tensor, dim: int) -> torch.Tensor:
    """The taps in ascending order along `dim` of v [..., H, W], zero padding, one rounding per product and per sum."""
    half = NTAPS // 2
    pad = (half, half, 0, 0) if dim == -1 else (0, 0, half, half)
    vp = F.pad(v, pad)
    n = v.shape[dim]
    acc = torch.zeros_like(v)
    for t in range(NTAPS):
        acc = acc + w[t] * vp.narrow(dim, t, n)
    return acc


def score_from_logp_explicit(logp: torch.Tensor, w: torch.Tensor | None = None) -> torch.Tensor:
    """log p [..., H, W] float32 -> the score map, in the written-out order."""
    w = density_taps(logp.dtype, logp.device) if w is None else w
    p = exp_explicit(logp)
    q = (p + 1e-6) * 10000
    dens = filter_explicit(filter_explicit(q, w, -1), w, -2)
    # the square root through float64: the float64 root rounded once is the correctly rounded float32 root (53 >= 2 x 24 + 2 bits), which
    # torch's float32 CPU sqrt is not on every build (a vector-library root, 1 ulp off on 0.7 % of the inputs where this was written)
    root = torch.sqrt((dens + 1e-8).double()).to(dens.dtype)
    return p * (1.0 / root)


def logp_explicit(logits: torch.Tensor) -> torch.Tensor:
    """logits [H, W] -> log p = (l - max) - log(sum exp(l - max))."""
    c = logits - logits.max()
    return c - torch.log(torch.exp(c).sum())


def scores_explicit(logits: torch.Tensor):
    logp = logp_explicit(logits)
    return logp, score_from_logp_explicit(logp)


def scores_library(logits: torch.Tensor):
    """Upstream's form: softmax over the image, F.conv2d with the taps (rows, then columns), `** -0.5`."""
    H, W = logits.shape
    p = logits.reshape(-1).softmax(dim=-1).reshape(1, 1, H, W)
    w = density_taps(logits.dtype, logits.device)[None, None]
    dx = F.conv2d((p + 1e-6) * 10000, w[..., None, :], padding=(0, NTAPS // 2))
    dens = F.conv2d(dx, w[..., None], padding=(NTAPS // 2, 0))
    return torch.log(p[0, 0]), (p * (dens + 1e-8) ** (-1 / 2))[0, 0]


def cut(score: torch.Tensor, k: int) -> torch.Tensor:
    """`torch.topk(score.flatten(), k)` with ties pinned: equal scores go to the lower flat index (topk leaves them open); k above the
    number of pixels raises, as topk does.  -> flat indices in descending score."""
    flat = score.reshape(-1)
    if k > flat.numel():
        raise RuntimeError(f"selected index k={k} out of range for {flat.numel()} pixels")
    return torch.sort(flat, descending=True, stable=True).indices[:k]


def grid_coords(idx: torch.Tensor, H: int, W: int, dtype=torch.float32) -> torch.Tensor:
    """get_grid's normalised pixel centres of the flat indices, (x, y): x = (2 j + 1) / W - 1."""
    i, j = torch.div(idx, W, rounding_mode="floor"), idx % W
    return torch.stack([(2 * j + 1).to(dtype) / W - 1, (2 * i + 1).to(dtype) / H - 1], -1)


def to_pixel_coords(g: torch.Tensor, H: int, W: int) -> torch.Tensor:
    return torch.stack([(g[..., 0] + 1) / 2 * W, (g[..., 1] + 1) / 2 * H], -1)


def select(score: torch.Tensor, k: int) -> dict:
    """The cut and the key-point rows on a score map [H, W]."""
    H, W = score.shape
    idx = cut(score, k)
    g = grid_coords(idx, H, W, score.dtype)
    return {"idx": idx, "grid": g, "keypoints": to_pixel_coords(g, H, W), "scores": score.reshape(-1)[idx]}


def describe(grid: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    """describe_keypoints: bilinear grid_sample (align_corners=False) of the description grid [256,H,W] at g [n,2] -> [n,256]."""
    return F.grid_sample(grid[None], g[None, None].to(grid), mode="bilinear", align_corners=False)[0, :, 0].t()


def normalize(image: torch.Tensor, dtype) -> torch.Tensor:
    x = image.to(dtype)
    return (x - torch.tensor(MEAN, dtype=dtype, device=x.device).view(1, 3, 1, 1)) / torch.tensor(STD, dtype=dtype, device=x.device).view(1, 3, 1, 1)


def extract(sd_detector: dict, sd_descriptor: dict, image: torch.Tensor, conf: dict, dtype=torch.float32, form=scores_explicit) -> dict:
    """image [1,3,H,W] RGB in [0,1] -> the wrapper's outputs (keypoints [n,2] pixels, scores [n], descriptors [n,256]) plus idx, the
    detector's accumulated `logits` per scale [h,w], `logp`, `score` [H,W], `desc2` [H/2,W/2,256] and `dense` [H,W,256]."""
    conf = {**DEFAULT_CONF, **conf}
    assert image.shape[0] == 1 and image.shape[1] == 3 and not conf["dense"]
    H, W = image.shape[2:]
    assert H % 8 == 0 and W % 8 == 0
    img = normalize(image, dtype)
    logits = [a[0, 0] for a in decode(sd_detector, img, "detector")]
    logp, score = form(logits[-1])
    out = select(score, int(conf["max_keypoints"]))
    grids = decode(sd_descriptor, img, "descriptor")
    out["descriptors"] = describe(grids[-1][0], out["grid"])
    out.update(logits=logits, logp=logp, score=score, desc2=grids[-2][0].permute(1, 2, 0), dense=grids[-1][0].permute(1, 2, 0))
    return out
