"""Numpy restatement of OpenCV 4.x SIFT (float pipeline, sigma 1.6, first octave -1) and of the wrapper stages of
imcui/hloc/extractors/sift.py, written from the algorithm's description: the definition csrc/sift.hip is tested against.

Staged: `pyramid`, `detect` (with a per-candidate trace of decision margins), `orientations`, `describe`, `wrapper_stages`.  Every stage
takes `dtype`: float64 is the yardstick, float32 rounds after every operation like the device and measures the format's own spread.
Conventions shared with the device: the Gaussian taps are float32 constants (computed in float64, normalised, rounded); the angle of
a gradient is atan2, and the BIN of an orientation-histogram sample is decided in float64 in both modes (`orientations`), so that a
float32 angle one ulp off a bin boundary cannot move a whole sample between bins.
"""
from __future__ import annotations

import math

import numpy as np

SIGMA, BORDER, MAX_STEPS, ORI_BINS = 1.6, 5, 5, 36
FLT_EPS = 1.1920929e-07
DEG = 57.29577951308232
RAD32 = np.float32(0.017453292519943295)


# ------------------------------------------------------------------ images
def seeded_image(h: int, w: int, seed: int = 0, oy: int = 0, ox: int = 0) -> np.ndarray:
    """Gray float32 image in [0,1]: structure at 4 / 8 / 16 / 48-pixel periods + 2 % noise.  (oy, ox) shifts the structure (not the noise
    seed's layout: the noise is a field of the canvas, indexed by absolute position), so two calls are crops of one canvas."""
    canvas = seeded_canvas(oy + h, ox + w, seed)
    return np.ascontiguousarray(canvas[oy : oy + h, ox : ox + w])


def seeded_canvas(h: int, w: int, seed: int = 0) -> np.ndarray:
    rng = np.random.default_rng(seed)
    big = 1024  # (the canvas, not the crop, fixes the random fields: every size up to 1024 is a crop of the same picture)
    while big < max(h, w):
        big *= 2
    yy, xx = np.mgrid[0:big, 0:big].astype(np.float64)
    img = np.zeros((big, big))
    for period, amp in ((4, 0.08), (8, 0.12), (16, 0.18), (48, 0.25)):
        # random blocky field of that period, smoothed by bilinear interpolation of a coarse grid
        gh = big // period + 2
        coarse = rng.random((gh, gh))
        fy, fx = yy / period, xx / period
        iy, ix = fy.astype(int), fx.astype(int)
        ty, tx = fy - iy, fx - ix
        ty, tx = ty * ty * (3 - 2 * ty), tx * tx * (3 - 2 * tx)
        f = (coarse[iy, ix] * (1 - ty) * (1 - tx) + coarse[iy, ix + 1] * (1 - ty) * tx + coarse[iy + 1, ix] * ty * (1 - tx) + coarse[iy + 1, ix + 1] * ty * tx)
        img += amp * (f - 0.5)
    img = 0.5 + img + 0.02 * rng.standard_normal((big, big))
    return np.clip(img, 0.0, 1.0).astype(np.float32)[:h, :w]


def to_u8(image: np.ndarray) -> np.ndarray:
    """[1,H,W] or [3,H,W] float32 in [0,1] -> uint8 [H,W]: kornia's rgb_to_grayscale in float32, then `(x * 255.0).astype(uint8)`."""
    image = np.asarray(image, dtype=np.float32)
    if image.shape[0] == 3:
        g = np.float32(0.299) * image[0] + np.float32(0.587) * image[1] + np.float32(0.114) * image[2]
    else:
        g = image[0]
    return (g * np.float32(255.0)).astype(np.uint8)


# ------------------------------------------------------------------ pyramid
def num_octaves(H: int, W: int) -> int:
    return int(np.rint(math.log2(2 * min(H, W)) - 2.0)) + 1


def gaussian_taps(sigma: float) -> np.ndarray:
    ks = int(np.rint(8.0 * sigma + 1.0)) | 1
    r = ks // 2
    k = [math.exp(-(i * i) / (2.0 * sigma * sigma)) for i in range(-r, r + 1)]
    s = 0.0
    for v in k:
        s += v
    return np.array([v / s for v in k], dtype=np.float32)


def reflect101(i: np.ndarray, n: int) -> np.ndarray:
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    i = np.mod(i, p)
    return np.where(i < n, i, p - i)


def blur(img: np.ndarray, sigma: float, dtype) -> np.ndarray:
    taps = gaussian_taps(sigma).astype(dtype)
    r = len(taps) // 2
    h, w = img.shape
    cols = reflect101(np.arange(-r, w + r), w)
    acc = taps[0] * img[:, cols[0:w]]
    for k in range(1, 2 * r + 1):
        acc = acc + taps[k] * img[:, cols[k : k + w]]
    rows = reflect101(np.arange(-r, h + r), h)
    out = taps[0] * acc[rows[0:h], :]
    for k in range(1, 2 * r + 1):
        out = out + taps[k] * acc[rows[k : k + h], :]
    return out.astype(dtype)


def upsample2(u8: np.ndarray) -> np.ndarray:
    """INTER_LINEAR to (2W, 2H): src = (dst + 0.5) / 2 - 0.5, clamped; exact in float32 (weights are quarters)."""
    src = u8.astype(np.float64)
    H, W = src.shape

    def axis(n):
        f = (np.arange(2 * n) + 0.5) * 0.5 - 0.5
        s = np.floor(f).astype(int)
        f = f - s
        lo = s < 0
        s[lo], f[lo] = 0, 0.0
        hi = s >= n - 1
        s[hi], f[hi] = n - 1, 0.0
        return s, np.minimum(s + 1, n - 1), f

    y0, y1, fy = axis(H)
    x0, x1, fx = axis(W)
    h0 = src[y0][:, x0] * (1 - fx) + src[y0][:, x1] * fx
    h1 = src[y1][:, x0] * (1 - fx) + src[y1][:, x1] * fx
    return h0 * (1 - fy)[:, None] + h1 * fy[:, None]


def level_sigmas(layers: int) -> list:
    k = 2.0 ** (1.0 / layers)
    sig = [SIGMA]
    for i in range(1, layers + 3):
        prev = (k ** (i - 1)) * SIGMA
        tot = prev * k
        sig.append(math.sqrt(tot * tot - prev * prev))
    return sig


def pyramid(u8: np.ndarray, layers: int = 4, dtype=np.float64) -> list:
    """uint8 [H,W] -> list over octaves of [layers+3, h, w]; every level blurred from the previous one."""
    H, W = u8.shape
    sig = level_sigmas(layers)
    base = blur(upsample2(u8).astype(dtype), math.sqrt(max(SIGMA * SIGMA - 4 * 0.25, 0.01)), dtype)
    out = []
    for o in range(num_octaves(H, W)):
        if o > 0:
            base = out[-1][layers][::2, ::2][: out[-1].shape[1] // 2, : out[-1].shape[2] // 2]
        if base.shape[0] < 1 or base.shape[1] < 1:
            break
        lv = [base]
        for i in range(1, layers + 3):
            lv.append(blur(lv[-1], sig[i], dtype))
        out.append(np.stack(lv))
    return out


def dog_of(octave: np.ndarray, dtype) -> np.ndarray:
    """DoG formed in float32 (what the device compares), then handed to the working dtype."""
    o32 = octave.astype(np.float32)
    return (o32[1:] - o32[:-1]).astype(dtype)


# ------------------------------------------------------------------ detection
def extrema(dog: np.ndarray, layers: int, contrast: float) -> np.ndarray:
    """-> [n,3] (layer, r, c) in scan order; 26-neighbour extrema of layers 1..layers, 5 pixels inside the border."""
    thr = math.floor(0.5 * contrast / layers * 255.0)
    L, h, w = dog.shape
    if h <= 2 * BORDER or w <= 2 * BORDER:
        return np.zeros((0, 3), int)
    v = dog[1 : layers + 1, BORDER : h - BORDER, BORDER : w - BORDER]
    mx = np.full(v.shape, -np.inf)
    mn = np.full(v.shape, np.inf)
    for dl in (-1, 0, 1):
        for dr in (-1, 0, 1):
            for dc in (-1, 0, 1):
                n = dog[1 + dl : layers + 1 + dl, BORDER + dr : h - BORDER + dr, BORDER + dc : w - BORDER + dc]
                mx = np.maximum(mx, n)
                mn = np.minimum(mn, n)
    is_ext = (np.abs(v) > thr) & (((v > 0) & (v >= mx)) | ((v < 0) & (v <= mn)))
    l, r, c = np.nonzero(is_ext)
    return np.stack([l + 1, r + BORDER, c + BORDER], 1)


def _solve3(A, dtype):
    """Gaussian elimination with partial pivoting on the augmented 3x4 system; None when a pivot is below FLT_EPSILON."""
    A = [[dtype(x) for x in row] for row in A]
    eps = dtype(FLT_EPS)
    if abs(A[1][0]) > abs(A[0][0]):
        A[0], A[1] = A[1], A[0]
    if abs(A[2][0]) > abs(A[0][0]):
        A[0], A[2] = A[2], A[0]
    if abs(A[0][0]) < eps:
        return None
    for i in (1, 2):
        f = A[i][0] / A[0][0]
        for k in range(1, 4):
            A[i][k] = A[i][k] - f * A[0][k]
    if abs(A[2][1]) > abs(A[1][1]):
        A[1], A[2] = A[2], A[1]
    if abs(A[1][1]) < eps:
        return None
    f = A[2][1] / A[1][1]
    for k in (2, 3):
        A[2][k] = A[2][k] - f * A[1][k]
    if abs(A[2][2]) < eps:
        return None
    x2 = A[2][3] / A[2][2]
    x1 = (A[1][3] - A[1][2] * x2) / A[1][1]
    x0 = (A[0][3] - A[0][2] * x2 - A[0][1] * x1) / A[0][0]
    return x0, x1, x2


def refine(dog: np.ndarray, o: int, l: int, r: int, c: int, layers: int, contrast: float, edge: float, dtype) -> dict:
    """adjustLocalExtrema.  -> dict(valid, o, l, r, c, xc, xr, xi, contr, size, x, y, edge_q, det, margins{offset, contrast, edge})."""
    L, h, w = dog.shape
    T = dtype
    is_ = T(1.0) / T(255.0)
    ds, cs = is_ * T(0.5), is_ * T(0.25)
    D = dog
    margins = {"offset": np.inf, "contrast": np.inf, "edge": np.inf}
    res = dict(valid=False, o=o, l=l, r=r, c=c, margins=margins)
    xc = xr = xi = T(0)
    converged = False
    for _ in range(MAX_STEPS):
        v = D[l, r, c]
        cl, cr, ru, rd, sp, sn = D[l, r, c - 1], D[l, r, c + 1], D[l, r - 1, c], D[l, r + 1, c], D[l - 1, r, c], D[l + 1, r, c]
        gx, gy, gs = (cr - cl) * ds, (rd - ru) * ds, (sn - sp) * ds
        v2 = v * T(2)
        dxx, dyy, dss = (cr + cl - v2) * is_, (rd + ru - v2) * is_, (sn + sp - v2) * is_
        dxy = (D[l, r + 1, c + 1] - D[l, r + 1, c - 1] - D[l, r - 1, c + 1] + D[l, r - 1, c - 1]) * cs
        dxs = (D[l + 1, r, c + 1] - D[l + 1, r, c - 1] - D[l - 1, r, c + 1] + D[l - 1, r, c - 1]) * cs
        dys = (D[l + 1, r + 1, c] - D[l + 1, r - 1, c] - D[l - 1, r + 1, c] + D[l - 1, r - 1, c]) * cs
        X = _solve3([[dxx, dxy, dxs, gx], [dxy, dyy, dys, gy], [dxs, dys, dss, gs]], T)
        if X is None:
            return res
        xc, xr, xi = -X[0], -X[1], -X[2]
        margins["offset"] = min(margins["offset"], *(abs(abs(float(t)) - 0.5) for t in (xc, xr, xi)))
        if abs(xc) < 0.5 and abs(xr) < 0.5 and abs(xi) < 0.5:
            converged = True
            break
        if not (abs(xc) < 7e8 and abs(xr) < 7e8 and abs(xi) < 7e8):
            return res
        c += int(np.rint(xc))
        r += int(np.rint(xr))
        l += int(np.rint(xi))
        if l < 1 or l > layers or c < BORDER or c >= w - BORDER or r < BORDER or r >= h - BORDER:
            return res
    if not converged:
        return res
    t = gx * xc + gy * xr + gs * xi
    contr = v * is_ + t * T(0.5)
    margins["contrast"] = abs(abs(float(contr)) * layers - contrast)
    tr = dxx + dyy
    det = dxx * dyy - dxy * dxy
    e = T(edge)
    edge_q = tr * tr * e - (e + T(1)) * (e + T(1)) * det
    margins["edge"] = min(abs(float(edge_q)), abs(float(det)) * float((e + 1) * (e + 1)))
    res.update(l=l, r=r, c=c, xc=xc, xr=xr, xi=xi, contr=contr, edge_q=edge_q, det=det)
    if abs(contr) * layers < contrast or det <= 0 or edge_q >= 0:
        return res
    sc = T(1 << o)
    res["size"] = T(SIGMA) * T(2.0) ** ((T(l) + xi) / T(layers)) * sc * T(2)
    res["x"], res["y"] = (T(c) + xc) * sc, (T(r) + xr) * sc
    res["valid"] = True
    return res


def detect(pyr: list, layers: int = 4, contrast: float = 0.0066667, edge: float = 10.0, dtype=np.float64) -> dict:
    """-> dict(extrema [n,4] (o, l, r, c) in detection order, refined: one `refine` record per extremum)."""
    ext, recs = [], []
    for o, octave in enumerate(pyr):
        dog = dog_of(octave, dtype)
        e = extrema(dog, layers, contrast)
        for l, r, c in e:
            ext.append((o, int(l), int(r), int(c)))
            recs.append(refine(dog, o, int(l), int(r), int(c), layers, contrast, edge, dtype))
    return {"extrema": np.array(ext, dtype=int).reshape(-1, 4), "refined": recs}


# ------------------------------------------------------------------ orientation
def orientation_hist(img: np.ndarray, r: int, c: int, scl, dtype) -> np.ndarray:
    """Smoothed 36-bin histogram around pixel (r, c) of `img` (the key-point's level); scl = size * 0.5 / 2^octave."""
    T = dtype
    h, w = img.shape
    scl = T(scl)
    radius = int(np.rint(T(4.5) * scl))
    sigma = T(1.5) * scl
    es = T(-1.0) / (T(2.0) * sigma * sigma)
    ii, jj = np.mgrid[-radius : radius + 1, -radius : radius + 1]
    y, x = (r + ii).ravel(), (c + jj).ravel()
    ok = (y > 0) & (y < h - 1) & (x > 0) & (x < w - 1)
    y, x, i2 = y[ok], x[ok], (ii * ii + jj * jj).ravel()[ok]
    im = img.astype(T)
    dx = im[y, x + 1] - im[y, x - 1]
    dy = im[y - 1, x] - im[y + 1, x]
    wgt = np.exp(i2.astype(T) * es)
    mag = np.sqrt(dx * dx + dy * dy)
    # the bin is decided in float64 on the exact differences of the stored values
    i64 = img.astype(np.float64)
    ang = np.arctan2(i64[y - 1, x] - i64[y + 1, x], i64[y, x + 1] - i64[y, x - 1]) * DEG
    ang = np.where(ang < 0, ang + 360.0, ang)
    b = np.rint(ang * 0.1).astype(int)
    b[b >= ORI_BINS] -= ORI_BINS
    raw = np.zeros(ORI_BINS, dtype=T)
    np.add.at(raw, b, (wgt * mag).astype(T))
    return ((np.roll(raw, 2) + np.roll(raw, -2)) * T(1 / 16) + (np.roll(raw, 1) + np.roll(raw, -1)) * T(4 / 16) + raw * T(6 / 16)).astype(T)


def hist_peaks(hist: np.ndarray, dtype):
    """-> (bins, angles in degrees, margins per bin): bins strictly above both neighbours and >= 0.8 max."""
    T = dtype
    hl, hr = np.roll(hist, 1), np.roll(hist, -1)
    thr = hist.max() * T(0.8)
    pk = (hist > hl) & (hist > hr) & (hist >= thr)
    margins = np.minimum(np.minimum(np.abs(hist - hl), np.abs(hist - hr)), np.abs(hist - thr)).astype(np.float64)
    bins = np.nonzero(pk)[0]
    angles = []
    for j in bins:
        b = T(j) + T(0.5) * (hl[j] - hr[j]) / (hl[j] - T(2) * hist[j] + hr[j])
        b = T(ORI_BINS) + b if b < 0 else (b - T(ORI_BINS) if b >= ORI_BINS else b)
        a = T(360.0) - T(10.0) * b
        if abs(a - T(360.0)) < FLT_EPS:
            a = T(0)
        angles.append(a)
    return bins, np.array(angles, dtype=T), margins


def orientations(pyr: list, recs: list, dtype=np.float64) -> dict:
    """Key-point table from refined records: one row per (valid candidate, peak), columns as the device's table
    (o, l, r, c, xc, xr, xi, response, size, angle, x, y); `hists` holds the smoothed histogram of every valid candidate."""
    rows, hists, owner = [], {}, []
    for k, q in enumerate(recs):
        if not q["valid"]:
            continue
        scl = dtype(q["size"]) * dtype(0.5) / dtype(1 << q["o"])
        hist = orientation_hist(pyr[q["o"]][q["l"]], q["r"], q["c"], scl, dtype)
        hists[k] = hist
        _, angles, _ = hist_peaks(hist, dtype)
        for a in angles:
            rows.append([q["o"], q["l"], q["r"], q["c"], q["xc"], q["xr"], q["xi"], abs(q["contr"]), q["size"], a, q["x"], q["y"]])
            owner.append(k)
    return {"table": np.array(rows, dtype=dtype).reshape(-1, 12), "hists": hists, "owner": np.array(owner, dtype=int)}


# ------------------------------------------------------------------ descriptor
def describe(img: np.ndarray, o: int, x, y, size, angle, dtype=np.float64) -> dict:
    """calcSIFTDescriptor on the key-point's level.  x, y, size in the doubled image's units (the table's), angle in degrees.
    -> dict(raw [128] after x 512 / norm, quant [128] uint8 values, round_margin: distance of the cvRound arguments to a half-integer)."""
    T = dtype
    h, w = img.shape
    inv = T(1.0) / T(1 << o)
    px, py, scl = T(x) * inv, T(y) * inv, T(size) * inv * T(0.5)
    ori = T(360.0) - T(angle)
    if abs(ori - T(360.0)) < FLT_EPS:
        ori = T(0)
    cx, cy = int(np.rint(px)), int(np.rint(py))
    hw = T(3.0) * scl
    rad_arg = hw * T(1.4142135623730951) * T(5.0) * T(0.5)
    radius = min(int(np.rint(rad_arg)), int(math.sqrt(float(h) * h + float(w) * w)))
    half = lambda v: abs(abs(float(v) - math.floor(float(v))) - 0.5)  # noqa: E731
    round_margin = min(half(px), half(py), half(rad_arg))
    ct, st = np.cos(ori * T(0.017453292519943295)) / hw, np.sin(ori * T(0.017453292519943295)) / hw
    ii, jj = np.mgrid[-radius : radius + 1, -radius : radius + 1]
    i, j = ii.ravel().astype(T), jj.ravel().astype(T)
    c_rot, r_rot = j * ct - i * st, j * st + i * ct
    rbin, cbin = r_rot + T(1.5), c_rot + T(1.5)
    yy, xx = cy + ii.ravel(), cx + jj.ravel()
    ok = (rbin > -1) & (rbin < 4) & (cbin > -1) & (cbin < 4) & (yy > 0) & (yy < h - 1) & (xx > 0) & (xx < w - 1)
    rbin, cbin, c_rot, r_rot, yy, xx = rbin[ok], cbin[ok], c_rot[ok], r_rot[ok], yy[ok], xx[ok]
    im = img.astype(T)
    dx, dy = im[yy, xx + 1] - im[yy, xx - 1], im[yy - 1, xx] - im[yy + 1, xx]
    ang = np.arctan2(dy, dx) * T(DEG)
    ang = np.where(ang < 0, ang + T(360.0), ang)
    mag = np.sqrt(dx * dx + dy * dy) * np.exp((c_rot * c_rot + r_rot * r_rot) * T(-0.125))
    obin = (ang - ori) * T(8.0 / 360.0)
    r0, c0, o0 = np.floor(rbin), np.floor(cbin), np.floor(obin)
    rbin, cbin, obin = rbin - r0, cbin - c0, obin - o0
    r0, c0, o0 = r0.astype(int), c0.astype(int), o0.astype(int)
    o0 = np.where(o0 < 0, o0 + 8, o0)
    o0 = np.where(o0 >= 8, o0 - 8, o0)
    o1 = (o0 + 1) & 7
    v_r1 = mag * rbin
    v_r0 = mag - v_r1
    v_rc11 = v_r1 * cbin
    v_rc10 = v_r1 - v_rc11
    v_rc01 = v_r0 * cbin
    v_rc00 = v_r0 - v_rc01
    hist = np.zeros(128, dtype=T)
    for rr, cc, vrc in ((r0, c0, v_rc00), (r0, c0 + 1, v_rc01), (r0 + 1, c0, v_rc10), (r0 + 1, c0 + 1, v_rc11)):
        m = (rr >= 0) & (rr <= 3) & (cc >= 0) & (cc <= 3)
        v1 = vrc * obin
        v0 = vrc - v1
        np.add.at(hist, ((rr * 4 + cc) * 8 + o0)[m], v0[m].astype(T))
        np.add.at(hist, ((rr * 4 + cc) * 8 + o1)[m], v1[m].astype(T))
    thr = np.sqrt((hist * hist).sum(dtype=T)) * T(0.2)
    hist = np.minimum(hist, thr)
    raw = hist * (T(512.0) / max(np.sqrt((hist * hist).sum(dtype=T)), T(FLT_EPS)))
    quant = np.clip(np.rint(raw), 0, 255)
    return {"raw": raw.astype(T), "quant": quant.astype(np.float32), "round_margin": round_margin}


def rootsift(x: np.ndarray, eps: float = 1e-6) -> np.ndarray:
    """L1 normalise, clip at eps, square root, L2 normalise (rows of x)."""
    x = np.asarray(x)
    x = x / np.maximum(np.abs(x).sum(-1, keepdims=True), eps)
    x = np.sqrt(np.maximum(x, eps))
    return x / np.maximum(np.sqrt((x * x).sum(-1, keepdims=True)), eps)


# ------------------------------------------------------------------ post-processing and wrapper stages
def filter_points(points, scales, angles, image_shape, nms_radius, scores=None) -> np.ndarray:
    """Per pixel keep the highest score (scale without scores), of those the lowest |angle|; nms_radius > 0: keep a pixel only when it
    holds the maximum of its (2 r + 1)^2 window.  -> kept indices, ascending."""
    h, w = image_shape
    ij = np.round(points - 0.5).astype(int)
    row, col = ij[:, 1], ij[:, 0]
    s = scales if scores is None else scores
    best = np.zeros((h, w))
    np.maximum.at(best, (row, col), s)
    keep = np.nonzero(best[row, col] == s)[0]
    low = np.full((h, w), np.inf)
    a = np.abs(angles[keep])
    np.minimum.at(low, (row[keep], col[keep]), a)
    keep = keep[low[row[keep], col[keep]] == a]
    if nms_radius > 0:
        grid = np.zeros((h, w))
        grid[row[keep], col[keep]] = s[keep]
        pad = np.full((h + 2 * nms_radius, w + 2 * nms_radius), -np.inf)
        pad[nms_radius : nms_radius + h, nms_radius : nms_radius + w] = grid
        mx = np.full((h, w), -np.inf)
        for dy in range(2 * nms_radius + 1):
            for dx in range(2 * nms_radius + 1):
                mx = np.maximum(mx, pad[dy : dy + h, dx : dx + w])
        keep = keep[(grid == mx)[row[keep], col[keep]]]
    return keep


def top_k_keep(scores: np.ndarray, k: int):
    """The k highest scores (ties to the earlier entry), returned in their original order.  -> (indices ascending, the cut fell on a tie)."""
    order = np.lexsort((np.arange(len(scores)), -np.asarray(scores, np.float64)))
    tie = bool(scores[order[k - 1]] == scores[order[k]])
    return np.sort(order[:k]), tie


def wrapper_stages(table: np.ndarray, image_shape, nfeatures: int, nms_radius, max_keypoints) -> dict:
    """OpenCV's removeDuplicated / retainBest / halving, then the wrapper: filter, top-k.  `table` rows as the device's (float32
    values).  -> dict(keep: surviving rows ascending, keypoints, scores, scales, oris; tie_at_cut: the top-k cut fell on equal scores)."""
    t = np.asarray(table, dtype=np.float32)
    n = len(t)
    x, y, size, ang, resp = t[:, 10], t[:, 11], t[:, 8], t[:, 9], t[:, 7]
    alive = np.ones(n, bool)
    # removeDuplicated: same x, y, size, angle -> the highest response stays (ties: the earlier row)
    order = np.lexsort((np.arange(n), -resp.astype(np.float64), ang, size, y, x))
    for a, b in zip(order[:-1], order[1:]):
        if x[a] == x[b] and y[a] == y[b] and size[a] == size[b] and ang[a] == ang[b]:
            alive[b] = False
    if nfeatures and nfeatures > 0 and alive.sum() > nfeatures:
        nth = np.sort(resp[alive])[::-1][nfeatures - 1]
        alive &= resp >= nth
    idx = np.nonzero(alive)[0]
    pts = np.stack([x[idx] * np.float32(0.5), y[idx] * np.float32(0.5)], 1)
    scales, oris, scores = size[idx] * np.float32(0.5), ang[idx] * RAD32, resp[idx]
    if nms_radius is not None and nms_radius >= 0:
        k = filter_points(pts, scales, oris, image_shape, int(nms_radius), scores=scores)
        idx, pts, scales, oris, scores = idx[k], pts[k], scales[k], oris[k], scores[k]
    tie = False
    if max_keypoints and max_keypoints > 0 and len(idx) > max_keypoints:
        k, tie = top_k_keep(scores, max_keypoints)
        idx, pts, scales, oris, scores = idx[k], pts[k], scales[k], oris[k], scores[k]
    return {"keep": idx, "keypoints": pts, "scores": scores, "scales": scales, "oris": oris, "tie_at_cut": bool(tie)}


# ------------------------------------------------------------------ end to end
def extract(image: np.ndarray, conf: dict | None = None, dtype=np.float64, pyr: list | None = None) -> dict:
    """[1|3,H,W] float in [0,1] -> the wrapper's outputs in detection order + the intermediate stages."""
    c = {"rootsift": True, "nms_radius": 0, "max_keypoints": 4096, "detection_threshold": 0.0066667, "edge_threshold": 10, "num_octaves": 4}
    c.update(conf or {})
    layers = int(c["num_octaves"])
    u8 = to_u8(image)
    if pyr is None:
        pyr = pyramid(u8, layers, dtype)
    det = detect(pyr, layers, float(c["detection_threshold"]), float(c["edge_threshold"]), dtype)
    ori = orientations(pyr, det["refined"], dtype)
    maxk = int(c["max_keypoints"]) if c["max_keypoints"] else 0
    sel = wrapper_stages(ori["table"], u8.shape, maxk, c["nms_radius"], maxk)
    desc = []
    for row in ori["table"][sel["keep"]].astype(np.float32):
        o, l = int(row[0]), int(row[1])
        desc.append(describe(pyr[o][l], o, row[10], row[11], row[8], row[9], dtype)["quant"])
    desc = np.array(desc, dtype=np.float32).reshape(-1, 128)
    if c["rootsift"]:
        desc = rootsift(desc.astype(dtype)).astype(np.float32)
    return {**sel, "descriptors": desc, "pyramid": pyr, "detect": det, "orient": ori}


# ------------------------------------------------------------------ ground truth without the restatement: shift consistency
SHIFT = (16, 32)  # (dy, dx): multiples of 2^4 keep the sampling grids of the first five octaves aligned
SHIFT_POS_TOL, SHIFT_SCALE_TOL, SHIFT_ORI_TOL, SHIFT_MARGIN = 0.5, 0.05, 0.1, 40.0


def shift_pair(h: int, w: int, seed: int = 3):
    """Two [1,h,w] crops of one seeded canvas, the second offset by SHIFT: content at (x, y) of the first is at (x - dx, y - dy) of the second."""
    canvas = seeded_canvas(h + SHIFT[0], w + SHIFT[1], seed)
    return canvas[None, :h, :w].copy(), canvas[None, SHIFT[0] :, SHIFT[1] :].copy()


def shift_consistency(a: dict, b: dict, shape, match01=None) -> dict:
    """a, b: outputs (keypoints [n,2], scales, oris, descriptors [n,128]) for the two crops of `shift_pair`.  Interior key-points of `a`
    (more than SHIFT_MARGIN from the borders of both crops) must be found in `b` at the shifted position with the same scale and
    orientation; `match01` (matches of a in b, -1 = none; e.g. from a mutual-NN matcher) must pair them with that very key-point.
    -> dict(interior, refound, share, matched_share)."""
    h, w = shape
    dy, dx = SHIFT
    ka, kb = np.asarray(a["keypoints"], np.float64), np.asarray(b["keypoints"], np.float64)
    m = SHIFT_MARGIN
    inner = (ka[:, 0] > dx + m) & (ka[:, 0] < w - m) & (ka[:, 1] > dy + m) & (ka[:, 1] < h - m)
    # only key-points of the first five octaves keep their sampling grid under this shift
    inner &= np.asarray(a["scales"]) < 1.6 * 2 * 2 ** 4
    refound = matched = 0
    for i in np.nonzero(inner)[0]:
        d = np.abs(kb - (ka[i] - (dx, dy))).max(1)
        ds = np.abs(np.asarray(b["scales"]) / a["scales"][i] - 1.0)
        do = np.abs(np.angle(np.exp(1j * (np.asarray(b["oris"], np.float64) - float(a["oris"][i])))))
        hit = np.nonzero((d < SHIFT_POS_TOL) & (ds < SHIFT_SCALE_TOL) & (do < SHIFT_ORI_TOL))[0]
        if len(hit):
            refound += 1
            if match01 is not None and int(match01[i]) in set(hit.tolist()):
                matched += 1
    n = int(inner.sum())
    return {"interior": n, "refound": refound, "share": refound / max(n, 1), "matched_share": matched / max(refound, 1)}


def mutual_nn(d0: np.ndarray, d1: np.ndarray) -> np.ndarray:
    """Mutual nearest neighbours on unit descriptors (rows) -> matches of d0 in d1 (-1 = none)."""
    sim = d0.astype(np.float64) @ d1.astype(np.float64).T
    n01, n10 = sim.argmax(1), sim.argmax(0)
    ok = n10[n01] == np.arange(len(d0))
    return np.where(ok, n01, -1)
