"""Thin Python host layer over the C ABI: handles, weight packing, workspaces, launches.

PyTorch-ROCm tensors in, tensors out.  Everything is enqueued on
``torch.cuda.current_stream()``; nothing here synchronises except where the reference's
ragged list outputs force a device->host read of the key-point counts, and LoFTR's default
windowed fine stage (`LoFTRHIP.forward`), which reads its match count back.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import keyword
import math
import threading

import numpy as np
import torch

from . import header
from .lib_loader import ImcuiHipError, load_library

SP_ORDER = ["conv1a", "conv1b", "conv2a", "conv2b", "conv3a", "conv3b", "conv4a", "conv4b", "convPa", "convPb", "convDa", "convDb"]

_handles: dict[int, "Handle"] = {}
_hlock = threading.Lock()


class Handle:
    def __init__(self, device_index: int):
        self.lib = load_library()
        self.device_index = device_index
        h = C.c_void_p()
        rc = self.lib.imcui_hip_create(device_index, C.byref(h))
        if rc != 0 or not h:
            raise ImcuiHipError(f"imcui_hip_create(device={device_index}) failed with {rc} (no usable HIP device?)")
        self.h = h

    def check(self, rc: int, what: str = ""):
        if rc != 0:
            msg = self.lib.imcui_hip_last_error(self.h)
            raise ImcuiHipError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")

    def call(self, fn, *args):
        """`fn(h, *args)` for an ABI function of this handle; a non-zero status raises, naming the C symbol."""
        self.check(fn(self.h, *args), fn.__name__)

    def launch(self, fn, *args, check: bool = True) -> int:
        """The one path of every stream-ordered ABI call: `fn(h, *args, stream)` on this handle's device and its current stream.  A
        non-zero status raises, naming the C symbol; with check=False it is returned instead (the probes' refusal tests)."""
        with torch.cuda.device(self.device_index):
            rc = fn(self.h, *args, _stream_ptr())
        if check:
            self.check(rc, fn.__name__)
        return rc


def get_handle(device: torch.device) -> Handle:
    if device.type != "cuda":
        raise ImcuiHipError(f"the HIP backend needs a ROCm device tensor, got device '{device}' (no CPU fallback)")
    idx = device.index if device.index is not None else torch.cuda.current_device()
    with _hlock:
        if idx not in _handles:
            _handles[idx] = Handle(idx)
        return _handles[idx]


def _stream_ptr() -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t: torch.Tensor | None) -> C.c_void_p:
    return C.c_void_p(0 if t is None else t.data_ptr())


PY_FIELD_NAMES = {"in": "inp"}  # descriptor fields of the header whose names are Python keywords -> their spelling here


def _desc_fields(struct: str) -> list:
    """`_fields_` of the ctypes class of a descriptor struct of include/imcui_hip.h, in the header's order and types."""
    fields = [(PY_FIELD_NAMES.get(name, name), t) for name, t in header.read().structs[struct]]
    for name, _ in fields:
        if keyword.iskeyword(name):
            raise ImcuiHipError(f"{struct}.{name} is a Python keyword: give it a spelling in PY_FIELD_NAMES")
    return fields


def _fill_desc(d, fields: dict, who: str):
    """The descriptor `d` with `fields` set: a device tensor becomes its pointer, None a null pointer, a host tensor is refused."""
    for k, v in fields.items():
        if isinstance(v, torch.Tensor):
            if v.device.type != "cuda":
                raise ImcuiHipError(f"{who}: field {k} must be a device tensor")
            v = v.data_ptr()
        elif v is None:
            v = 0
        setattr(d, k, v)
    return d


def _route_table(device: torch.device, fn_name: str) -> dict:
    """{route: value} of a per-route table of the device's handle (launch counts, feature masks), zero entries left out."""
    hd = get_handle(device)
    fn = getattr(hd.lib, fn_name)
    n = fn(hd.h, None, 0)
    buf = (C.c_int * n)()
    fn(hd.h, buf, n)
    return {r: c for r, c in enumerate(buf) if c}


def _as_f32_host(t) -> np.ndarray:
    if isinstance(t, torch.Tensor):
        t = t.detach().to("cpu", torch.float32).contiguous().numpy()
    return np.ascontiguousarray(t, dtype=np.float32)


def _pad_rows(t: torch.Tensor, n: int, device: torch.device) -> torch.Tensor:
    """[B, m, ...] -> float32 [B, n, ...] on `device`, rows m.. zero (the tensor itself, made contiguous, when m == n)."""
    if t.shape[1] == n:
        return t.contiguous().float()
    shape = list(t.shape)
    shape[1] = n
    o = torch.zeros(shape, dtype=torch.float32, device=device)
    o[:, : t.shape[1]] = t
    return o


def _pack_arrays(arrs: list, n_floats: int, pack_call, *lead) -> torch.Tensor:
    """`pack_call(*lead, pointers to the float32 host arrays `arrs`, packed)` -> the float32 buffer (host) it filled."""
    packed = np.zeros(n_floats, dtype=np.float32)
    tp = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
    rc = pack_call(*lead, tp, packed.ctypes.data)
    if rc != 0:
        raise ImcuiHipError(f"{pack_call.__name__} failed ({rc})")
    return torch.from_numpy(packed)


def _pack_named(kind: str, layout_name: str, names: list, shapes: dict, state_dict: dict, n_floats: int, pack_call, *lead) -> torch.Tensor:
    """The strict packer of a network whose library entry takes its tensors by name order: `state_dict` (already without the keys the
    caller ignores) must hold exactly `names`, each with its shape in `shapes`; `pack_call(*lead, tensor pointers, packed)` fills the
    float32 buffer (host) that is returned."""
    missing = [n for n in names if n not in state_dict]
    extra = sorted(set(state_dict) - set(names))
    if missing or extra:
        raise ImcuiHipError(f"{kind} state dict does not match {layout_name} layout: missing {missing[:4]}, unexpected {extra[:4]}")
    arrs = []
    for n in names:
        a = _as_f32_host(state_dict[n])
        if a.shape != shapes[n]:
            raise ImcuiHipError(f"{kind} state dict: '{n}' has shape {a.shape}, expected {shapes[n]}")
        arrs.append(a)
    return _pack_arrays(arrs, n_floats, pack_call, *lead)


def _same_device(packed: torch.Tensor, image: torch.Tensor) -> None:
    if packed.device != image.device:
        raise ImcuiHipError("packed weights and image live on different devices")


def _sparse_outputs(B: int, kcap: int, dim: int, dev: torch.device):
    """The fixed-stride outputs of an extractor, uninitialised: keypoints [B,kcap,2], scores [B,kcap], descriptors [B,kcap,dim],
    num_keypoints [B] int32, status [1] int32, and the dict that returns them."""
    kpts = torch.empty((B, kcap, 2), dtype=torch.float32, device=dev)
    scores = torch.empty((B, kcap), dtype=torch.float32, device=dev)
    desc = torch.empty((B, kcap, dim), dtype=torch.float32, device=dev)
    nk = torch.empty((B,), dtype=torch.int32, device=dev)
    status = torch.empty((1,), dtype=torch.int32, device=dev)
    return kpts, scores, desc, nk, status, {"keypoints": kpts, "scores": scores, "descriptors": desc, "num_keypoints": nk, "status": status}


_owner = threading.local()


@contextlib.contextmanager
def workspace_owner(table: dict):
    """Inside the block, scratch handed out on this thread comes from `table` (one buffer per (`_Workspace`, device)) instead of the
    per-stream buffers.  A captured graph enters it around its warm-up and capture and keeps `table` as an attribute: the graph owns its
    scratch, no stream or other graph can grow or re-use it, and it is freed together with the graph."""
    prev = getattr(_owner, "table", None)
    _owner.table = table
    try:
        yield
    finally:
        _owner.table = prev


class _Workspace:
    """Caller-provided scratch of the C ABI: one grow-only byte buffer per (device, stream), or per device in the table of the active
    `workspace_owner`.

    Kernels of one stream execute in order, so a buffer is only ever shared by launches that are ordered anyway; two streams (two Gradio
    worker threads, a side stream) get separate buffers and cannot overwrite each other's scratch while kernels are in flight.  A HIP-graph
    capture must run inside a `workspace_owner`: a buffer handed out during the capture is baked into the graph, and a later request that
    would have to re-allocate it raises instead of freeing memory the graph still replays on."""

    def __init__(self):
        self._bufs: dict[tuple[int, int], tuple[torch.Tensor, bool]] = {}  # (device, stream) -> (buffer, pinned)
        self._lock = threading.Lock()

    @contextlib.contextmanager
    def use(self, nbytes: int, device: torch.device):
        """A buffer of at least `nbytes` bytes, the lock held until the block (the launch that reads it) ends."""
        idx = device.index if device.index is not None else torch.cuda.current_device()
        capturing = torch.cuda.is_current_stream_capturing()
        table = getattr(_owner, "table", None)
        if table is not None:
            key = (self, idx)
        elif capturing:
            raise ImcuiHipError("HIP-graph capture outside backend.workspace_owner: the graph's scratch would be a stream's buffer that later calls may free")
        else:
            table, key = self._bufs, (idx, torch.cuda.current_stream(device).cuda_stream)
        with self._lock:
            buf, pinned = table.get(key, (None, False))
            if buf is None or buf.numel() < nbytes:
                if pinned:
                    raise ImcuiHipError(f"workspace of a captured HIP graph ({buf.numel()} B) cannot grow to {int(nbytes)} B: "
                                        "capture the graph after a warm-up at the largest shape")
                buf = None
                table.pop(key, None)
                buf = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
            table[key] = (buf, pinned or capturing)
            yield buf


# ------------------------------------------------------------------ SuperPoint
def pack_superpoint(state_dict: dict) -> torch.Tensor:
    """Upstream SuperPoint state dict -> packed float32 buffer (host)."""
    lib = load_library()
    ws = [_as_f32_host(state_dict[f"{n}.weight"]) for n in SP_ORDER]
    bs = [_as_f32_host(state_dict[f"{n}.bias"]) for n in SP_ORDER]
    expect = {"conv1a": (64, 1, 3, 3), "convPb": (65, 256, 1, 1), "convDb": (256, 256, 1, 1)}
    for n, shp in expect.items():
        if tuple(state_dict[f"{n}.weight"].shape) != shp:
            raise ImcuiHipError(f"unexpected shape for {n}.weight: {tuple(state_dict[f'{n}.weight'].shape)}")
    packed = np.zeros(lib.imcui_hip_superpoint_packed_floats(), dtype=np.float32)
    wp = (C.c_void_p * 12)(*[w.ctypes.data for w in ws])
    bp = (C.c_void_p * 12)(*[b.ctypes.data for b in bs])
    rc = lib.imcui_hip_superpoint_pack_weights(wp, bp, packed.ctypes.data)
    if rc != 0:
        raise ImcuiHipError(f"imcui_hip_superpoint_pack_weights failed ({rc})")
    return torch.from_numpy(packed)


SP_TOPK_MAX = 16384  # on-chip top-k sorter of sp_topk_kernel (csrc/superpoint.hip)


class SuperPointHIP:
    def __init__(self):
        self._ws = _Workspace()

    def forward(self, packed: torch.Tensor, image: torch.Tensor, conf: dict, want_score_map: bool = False, kcap: int | None = None):
        """image [B,1,H,W] float32 on the GPU.  Returns dict of fixed-stride tensors + counts.

        Never synchronises: `status` [1] int32 is the selection status word on the device (0 = fine; bit 1 =
        `kcap` was too small, which only max_keypoints = -1 with exactly tied scores can cause) -- callers that
        read `num_keypoints` on the host anyway (the ragged plugin path) read it in the same copy."""
        hd = get_handle(image.device)
        _same_device(packed, image)
        lib = hd.lib
        image = image.contiguous().float()
        B, Cc, H, W = image.shape
        if Cc != 1:
            raise ImcuiHipError(f"SuperPoint expects a 1-channel image, got {Cc}")
        nms = int(conf["nms_radius"])
        maxk = int(conf["max_keypoints"])
        if maxk > SP_TOPK_MAX and H * W > SP_TOPK_MAX:
            raise ImcuiHipError(f"max_keypoints={maxk} exceeds the on-chip top-k sorter ({SP_TOPK_MAX}); use -1 to keep every key-point")
        if kcap is None:
            kcap = lib.imcui_hip_superpoint_max_keypoints_bound(H, W, nms) if maxk < 0 else max(1, min(maxk, H * W))
        dev = image.device
        kpts, scores, desc, nk, status, out = _sparse_outputs(B, kcap, 256, dev)
        smap = torch.empty((B, H, W), dtype=torch.float32, device=dev) if want_score_map else None
        with self._ws.use(lib.imcui_hip_superpoint_workspace_bytes(B, H, W, nms), dev) as ws:
            hd.launch(
                lib.imcui_hip_superpoint_forward, _ptr(packed), _ptr(image), B, H, W, nms, float(conf["keypoint_threshold"]),
                int(conf["remove_borders"]), maxk, int(bool(conf.get("fix_sampling", False))), kcap,
                _ptr(kpts), _ptr(scores), _ptr(desc), _ptr(nk), _ptr(status), _ptr(smap), _ptr(ws), ws.numel(),
            )  # fmt: skip
        if want_score_map:
            out["score_map"] = smap
        return out

    def select_probe(self, nms: torch.Tensor, keypoint_threshold: float, remove_borders: int, max_keypoints: int, kcap: int,
                     cand_cap: int | None = None, out: dict | None = None, check: bool = True):
        """Test entry: the selection stage of `forward` alone (imcui_hip_superpoint_select_probe) on the post-NMS map nms [B,H,W].
        `out` = caller's (pre-filled) keypoints [B,kcap,2], scores [B,kcap], num_keypoints [B] int32, status [1] int32; made here
        when None.  Returns `out`; with check=False a refused call returns its negative status instead of raising."""
        hd = get_handle(nms.device)
        lib = hd.lib
        nms = nms.contiguous().float()
        B, H, W = nms.shape
        cand_cap = H * W if cand_cap is None else int(cand_cap)
        if out is None:
            kpts, scores, _, nk, status, out = _sparse_outputs(B, max(1, kcap), 1, nms.device)
            del out["descriptors"]
        args = (_ptr(nms), B, H, W, float(keypoint_threshold), int(remove_borders), int(max_keypoints), int(kcap), cand_cap,
                _ptr(out["keypoints"]), _ptr(out["scores"]), _ptr(out["num_keypoints"]), _ptr(out["status"]))  # fmt: skip
        with self._ws.use(max(256, lib.imcui_hip_superpoint_select_workspace_bytes(B, H, W, cand_cap)), nms.device) as ws:
            rc = hd.launch(lib.imcui_hip_superpoint_select_probe, *args, _ptr(ws), ws.numel(), check=check)
        return out if rc == 0 else rc


# ------------------------------------------------------------------ DISK
def disk_tensor_names() -> list[str]:
    lib = load_library()
    return [lib.imcui_hip_disk_tensor_name(i).decode() for i in range(lib.imcui_hip_disk_num_tensors())]


def disk_tensor_shapes() -> dict:
    """kornia DISK's state-dict shapes (Unet(in_features=3, size=5, down=[16, 32, 64, 64, 64], up=[64, 64, 64, 129]))."""
    blocks = [("unet.path_down.0.1", 3, 16), ("unet.path_down.1.1", 16, 32), ("unet.path_down.2.1", 32, 64), ("unet.path_down.3.1", 64, 64),
              ("unet.path_down.4.1", 64, 64), ("unet.path_up.0.conv", 128, 64), ("unet.path_up.1.conv", 128, 64), ("unet.path_up.2.conv", 96, 64),
              ("unet.path_up.3.conv", 80, 129)]  # fmt: skip
    shapes = {}
    for i, (name, cin, cout) in enumerate(blocks):
        if i > 0:
            shapes[f"{name}.1.weight"] = (cin,)
        shapes[f"{name}.3.weight"] = (cout, cin, 5, 5)
        shapes[f"{name}.3.bias"] = (cout,)
    return shapes


def pack_disk(state_dict: dict) -> torch.Tensor:
    """kornia DISK state dict (the `["extractor"]` entry of a cvlab-epfl/disk checkpoint) -> packed float32 buffer (host).
    Strict: every key consumed exactly once, every shape checked."""
    lib = load_library()
    return _pack_named("DISK", "kornia's", disk_tensor_names(), disk_tensor_shapes(), state_dict, lib.imcui_hip_disk_packed_floats(),
                       lib.imcui_hip_disk_pack_weights)


def disk_check_args(image_shape, window: int, pad_if_not_divisible: bool) -> None:
    """The refusals of kornia's DISK.forward / nms, raised before anything is launched."""
    if len(image_shape) != 4 or image_shape[1] != 3:
        raise ValueError(f"DISK expects an RGB image [B,3,H,W], got shape {tuple(image_shape)}")
    if int(window) % 2 != 1:
        raise ValueError(f"window_size has to be odd, got {window}")
    H, W = image_shape[2:]
    if not pad_if_not_divisible and (H % 16 or W % 16):
        raise ValueError(f"Input image shape must be divisible by 16 (got {tuple(image_shape)}); set pad_if_not_divisible")


class DiskHIP:
    def __init__(self):
        self._ws = _Workspace()

    def forward(self, packed: torch.Tensor, image: torch.Tensor, conf: dict, want_heatmap: bool = False, kcap: int | None = None):
        """image [B,3,H,W] float32 on the GPU -> fixed-stride outputs, no host synchronisation: keypoints [B,K,2] (row-major order),
        scores [B,K], descriptors [B,K,128], num_keypoints [B] int32, status [1] int32 (bit 1: `kcap` too small), heatmap [B,H,W]
        when asked.  K = max_keypoints, or the exact NMS bound when max_keypoints is None."""
        window, pad = int(conf["nms_window_size"]), bool(conf["pad_if_not_divisible"])
        disk_check_args(tuple(image.shape), window, pad)
        hd = get_handle(image.device)
        _same_device(packed, image)
        lib = hd.lib
        image = image.contiguous().float()
        B, _, H, W = image.shape
        maxk = conf.get("max_keypoints")
        maxk = -1 if maxk is None or int(maxk) < 0 else int(maxk)
        bound = lib.imcui_hip_disk_max_keypoints_bound(H, W, window)
        if kcap is None:
            kcap = bound if maxk < 0 else max(1, min(maxk, bound))
        dev = image.device
        kpts, scores, desc, nk, status, out = _sparse_outputs(B, kcap, 128, dev)
        heat = torch.empty((B, H, W), dtype=torch.float32, device=dev) if want_heatmap else None
        with self._ws.use(lib.imcui_hip_disk_workspace_bytes(B, H, W), dev) as ws:
            hd.launch(
                lib.imcui_hip_disk_forward, _ptr(packed), _ptr(image), B, H, W, int(pad), window, float(conf["detection_threshold"]), maxk, kcap,
                _ptr(kpts), _ptr(scores), _ptr(desc), _ptr(nk), _ptr(status), _ptr(heat), _ptr(ws), ws.numel(),
            )  # fmt: skip
        if want_heatmap:
            out["heatmap"] = heat
        return out

    def select_probe(self, heat: torch.Tensor, window: int, threshold: float, max_keypoints: int | None, kcap: int, ccap: int | None = None,
                     out: dict | None = None, check: bool = True):
        """Test entry: the detection stage of `forward` alone (imcui_hip_disk_select_probe) on the heat map heat [B,H,W].  `out` = caller's
        (pre-filled) keypoints [B,kcap,2], scores [B,kcap], num_keypoints [B] int32, status [1] int32; made here when None.  Returns
        `out`; with check=False a refused call returns its negative status instead of raising."""
        hd = get_handle(heat.device)
        lib = hd.lib
        heat = heat.contiguous().float()
        B, H, W = heat.shape
        ccap = H * W if ccap is None else int(ccap)
        maxk = -1 if max_keypoints is None or int(max_keypoints) < 0 else int(max_keypoints)
        if out is None:
            kpts, scores, _, nk, status, out = _sparse_outputs(B, max(1, kcap), 1, heat.device)
            del out["descriptors"]
        args = (_ptr(heat), B, H, W, int(window), float(threshold), maxk, int(kcap), ccap,
                _ptr(out["keypoints"]), _ptr(out["scores"]), _ptr(out["num_keypoints"]), _ptr(out["status"]))  # fmt: skip
        with self._ws.use(max(256, lib.imcui_hip_disk_select_workspace_bytes(B, H, W, ccap)), heat.device) as ws:
            rc = hd.launch(lib.imcui_hip_disk_select_probe, *args, _ptr(ws), ws.numel(), check=check)
        return out if rc == 0 else rc


# ------------------------------------------------------------------ XFeat
XFEAT_DETECTION_THRESHOLD = 0.05  # upstream XFeat.__init__'s default: imcui/hloc/extractors/xfeat.py never passes its `keypoint_threshold`


def xfeat_tensor_names() -> list[str]:
    lib = load_library()
    return [lib.imcui_hip_xfeat_tensor_name(i).decode() for i in range(lib.imcui_hip_xfeat_num_tensors())]


def xfeat_tensor_shapes() -> dict:
    """XFeatModel's state-dict shapes (verlab/accelerated_features), without the `num_batches_tracked` counters and `fine_matcher.*`."""
    blocks = [
        ("block1", [(1, 4, 3), (4, 8, 3), (8, 8, 3), (8, 24, 3)], None),
        ("block2", [(24, 24, 3), (24, 24, 3)], None),
        ("block3", [(24, 64, 3), (64, 64, 3), (64, 64, 1)], None),
        ("block4", [(64, 64, 3), (64, 64, 3), (64, 64, 3)], None),
        ("block5", [(64, 128, 3), (128, 128, 3), (128, 128, 3), (128, 64, 1)], None),
        ("block_fusion", [(64, 64, 3), (64, 64, 3)], (64, 64)),
        ("heatmap_head", [(64, 64, 1), (64, 64, 1)], (64, 1)),
        ("keypoint_head", [(64, 64, 1), (64, 64, 1), (64, 64, 1)], (64, 65)),
    ]
    shapes = {"skip1.1.weight": (24, 1, 1, 1), "skip1.1.bias": (24,)}
    for name, layers, last in blocks:
        for i, (cin, cout, k) in enumerate(layers):
            shapes[f"{name}.{i}.layer.0.weight"] = (cout, cin, k, k)
            shapes[f"{name}.{i}.layer.1.running_mean"] = (cout,)
            shapes[f"{name}.{i}.layer.1.running_var"] = (cout,)
        if last is not None:
            shapes[f"{name}.{len(layers)}.weight"] = (last[1], last[0], 1, 1)
            shapes[f"{name}.{len(layers)}.bias"] = (last[1],)
    return shapes


def pack_xfeat(state_dict: dict) -> torch.Tensor:
    """XFeatModel state dict (a real `xfeat.pt`) -> packed float32 buffer (host); BatchNorm (eval, no affine part) is folded into the
    convolutions by the packer.  `fine_matcher.*` (the semi-dense refinement MLP) and the `num_batches_tracked` counters are accepted
    and ignored; every other key is consumed exactly once and every shape checked."""
    lib = load_library()
    own = {k: v for k, v in state_dict.items() if not k.startswith("fine_matcher.") and not k.endswith("num_batches_tracked")}
    return _pack_named("XFeat", "upstream's", xfeat_tensor_names(), xfeat_tensor_shapes(), own, lib.imcui_hip_xfeat_packed_floats(),
                       lib.imcui_hip_xfeat_pack_weights)


def xfeat_check_args(image_shape) -> None:
    """Refusals raised before anything is launched: upstream resizes to H // 32 * 32 x W // 32 * 32, which has to be non-empty."""
    if len(image_shape) != 4 or image_shape[1] not in (1, 3):
        raise ValueError(f"XFeat expects an image [B,1,H,W] or [B,3,H,W], got shape {tuple(image_shape)}")
    if image_shape[2] < 32 or image_shape[3] < 32:
        raise ValueError(f"XFeat needs images of at least 32 x 32, got {tuple(image_shape[2:])}")


class XFeatHIP:
    def __init__(self):
        self._ws = _Workspace()

    def forward(self, packed: torch.Tensor, image: torch.Tensor, conf: dict, want_dense: bool = False, kcap: int | None = None,
                threshold: float = XFEAT_DETECTION_THRESHOLD):
        """image [B,1|3,H,W] float32 on the GPU -> fixed-stride outputs in descending score order, no host synchronisation: keypoints
        [B,K,2], scores [B,K], descriptors [B,K,64], num_keypoints [B] int32, status [1] int32 (bit 1: `kcap` too small); with
        `want_dense` also kpt_heat [B,Hr,Wr], reliability [B,Hr/8,Wr/8], feats_norm [B,Hr/8,Wr/8,64].  `max_keypoints` is Python's
        `[:top_k]` per image (-1 drops the lowest score); K = the NMS bound, cut to max_keypoints when that is not negative."""
        xfeat_check_args(tuple(image.shape))
        hd = get_handle(image.device)
        _same_device(packed, image)
        lib = hd.lib
        image = image.contiguous().float()
        B, Cc, H, W = image.shape
        top_k = int(conf["max_keypoints"])
        bound = lib.imcui_hip_xfeat_max_keypoints_bound(H, W)
        if kcap is None:
            kcap = bound if top_k < 0 else max(1, min(top_k, bound))
        dev = image.device
        Hr, Wr = H // 32 * 32, W // 32 * 32
        kpts, scores, desc, nk, status, out = _sparse_outputs(B, kcap, 64, dev)
        heat = torch.empty((B, Hr, Wr), dtype=torch.float32, device=dev) if want_dense else None
        rel = torch.empty((B, Hr // 8, Wr // 8), dtype=torch.float32, device=dev) if want_dense else None
        m1 = torch.empty((B, Hr // 8, Wr // 8, 64), dtype=torch.float32, device=dev) if want_dense else None
        with self._ws.use(lib.imcui_hip_xfeat_workspace_bytes(B, H, W), dev) as ws:
            hd.launch(
                lib.imcui_hip_xfeat_forward, _ptr(packed), _ptr(image), B, Cc, H, W, float(threshold), top_k, kcap,
                _ptr(kpts), _ptr(scores), _ptr(desc), _ptr(nk), _ptr(status), _ptr(heat), _ptr(rel), _ptr(m1), _ptr(ws), ws.numel(),
            )  # fmt: skip
        if want_dense:
            out.update(kpt_heat=heat, reliability=rel, feats_norm=m1)
        return out

    def sample_probe(self, kpt_heat: torch.Tensor, reliability: torch.Tensor, feats: torch.Tensor, xy: torch.Tensor):
        """The kernel's sampling rules at integer pixels xy [n,2] (x, y) of kpt_heat [H,W]: nearest(kpt_heat) [n], bilinear(reliability
        [H/8,W/8]) [n], bicubic(feats [H/8,W/8,64]) [n,64] -- the test entry imcui_hip_xfeat_sample_probe."""
        hd = get_handle(kpt_heat.device)
        H, W = kpt_heat.shape
        dev = kpt_heat.device
        if tuple(reliability.shape) != (H // 8, W // 8) or tuple(feats.shape) != (H // 8, W // 8, 64):
            raise ValueError(f"reliability {tuple(reliability.shape)} / feats {tuple(feats.shape)} do not match a {H} x {W} key-point map")
        xy = xy.to(dev, torch.int32).contiguous()
        n = xy.shape[0]
        near = torch.empty((n,), dtype=torch.float32, device=dev)
        bil = torch.empty((n,), dtype=torch.float32, device=dev)
        cub = torch.empty((n, 64), dtype=torch.float32, device=dev)
        hd.launch(hd.lib.imcui_hip_xfeat_sample_probe, _ptr(kpt_heat.contiguous().float()), _ptr(reliability.contiguous().float()),
                  _ptr(feats.contiguous().float()), H, W, _ptr(xy), n, _ptr(near), _ptr(bil), _ptr(cub))  # fmt: skip
        return near, bil, cub


# ------------------------------------------------------------------ LiftFeat
LIFTFEAT_GROUPS = ("skip1", "block1", "block2", "block3", "block4", "block5", "block_fusion", "keypoint_head", "normal_head", "feature_boost")
LIFTFEAT_ALIGN_CORNERS, LIFTFEAT_SLOPE = 1, 0.1  # the up-sampling stages of the normal head (tests/liftfeat_reference.py, TABLE)


def liftfeat_config(sd: dict) -> dict:
    """Widths, depth and optional parts of the lifting network from the checkpoint's shapes and keys; a key group the layout does not
    know and a trunk tensor whose width differs from XFeat's are refused by name."""
    for k in sd:
        if k.split(".")[0] not in LIFTFEAT_GROUPS:
            raise ImcuiHipError(f"LiftFeat state dict: '{k}' belongs to no known key group ({', '.join(LIFTFEAT_GROUPS)})")
    trunk = xfeat_tensor_shapes()
    for k, v in sd.items():
        if k in trunk and tuple(v.shape) != trunk[k]:
            raise ImcuiHipError(f"LiftFeat state dict: '{k}' has shape {tuple(v.shape)}, XFeat's trunk has {trunk[k]}")
    fb = "feature_boost"

    def out_width(key):
        if f"{key}.weight" not in sd:
            raise ImcuiHipError(f"LiftFeat state dict: '{key}.weight' is missing")
        return int(sd[f"{key}.weight"].shape[0])

    layers = sorted({int(k.split(".")[2]) for k in sd if k.startswith(f"{fb}.layers.")})
    if not layers or layers != list(range(len(layers))):
        raise ImcuiHipError(f"LiftFeat state dict: '{fb}.layers' must be numbered 0 .. n - 1, got {layers}")
    kenc = any(k.startswith(f"{fb}.kenc.") for k in sd)
    cfg = {"kenc": int(kenc), "ffn": out_width(f"{fb}.layers.0.ffn.0"), "denc": out_width(f"{fb}.denc.0"), "nenc1": out_width(f"{fb}.nenc.0"),
           "nenc2": out_width(f"{fb}.nenc.2"), "kenc1": out_width(f"{fb}.kenc.0") if kenc else 0, "kenc2": out_width(f"{fb}.kenc.2") if kenc else 0,
           "n_layers": len(layers)}  # fmt: skip
    if load_library().imcui_hip_liftfeat_packed_floats(liftfeat_cfg_array(cfg)) == 0:
        raise ImcuiHipError(f"LiftFeat: configuration {cfg} is not supported (hidden widths: multiples of 32 up to 128, second hidden width 32 or 64, "
                            "1 .. 8 layers)")  # fmt: skip
    return cfg


def liftfeat_cfg_array(cfg: dict):
    return (C.c_int * 8)(cfg["kenc"], cfg["ffn"], cfg["denc"], cfg["nenc1"], cfg["nenc2"], cfg["kenc1"], cfg["kenc2"], cfg["n_layers"])


def liftfeat_tensor_names(cfg: dict) -> list[str]:
    lib, ca = load_library(), liftfeat_cfg_array(cfg)
    return [lib.imcui_hip_liftfeat_tensor_name(ca, i).decode() for i in range(lib.imcui_hip_liftfeat_num_tensors(ca))]


def liftfeat_tensor_shapes(cfg: dict) -> dict:
    shapes = {k: v for k, v in xfeat_tensor_shapes().items() if not k.startswith("heatmap_head.")}
    for s, c in enumerate((64, 32, 16)):
        shapes[f"normal_head.{s}.conv.weight"] = (c // 2, c, 3, 3)
        for k in ("conv.bias", "bn.weight", "bn.bias", "bn.running_mean", "bn.running_var"):
            shapes[f"normal_head.{s}.{k}"] = (c // 2,)
    shapes["normal_head.3.weight"], shapes["normal_head.3.bias"] = (3, 8, 1, 1), (3,)

    def lin(stem, cin, cout):
        shapes[f"{stem}.weight"], shapes[f"{stem}.bias"] = (cout, cin), (cout,)

    fb = "feature_boost"
    encoders = {"denc": (64, cfg["denc"], 64), "nenc": (192, cfg["nenc1"], cfg["nenc2"], 64)}
    if cfg["kenc"]:
        encoders["kenc"] = (65, cfg["kenc1"], cfg["kenc2"], 64)
    for name, w in encoders.items():
        for i in range(len(w) - 1):
            lin(f"{fb}.{name}.{2 * i}", w[i], w[i + 1])
    for i in range(cfg["n_layers"]):
        p = f"{fb}.layers.{i}"
        for n in ("q", "k", "v", "proj"):
            lin(f"{p}.attn.{n}", 64, 64)
        lin(f"{p}.ffn.0", 64, cfg["ffn"])
        lin(f"{p}.ffn.2", cfg["ffn"], 64)
        for n in ("norm1", "norm2"):
            shapes[f"{p}.{n}.weight"], shapes[f"{p}.{n}.bias"] = (64,), (64,)
    lin(f"{fb}.final_proj", 64, 64)
    return shapes


def pack_liftfeat(state_dict: dict):
    """LiftFeat state dict -> (packed float32 buffer (host), cfg).  `num_batches_tracked` counters are dropped; every other key is consumed
    exactly once and every shape checked."""
    lib = load_library()
    sd = {k: v for k, v in state_dict.items() if not k.endswith("num_batches_tracked")}
    cfg = liftfeat_config(sd)
    ca = liftfeat_cfg_array(cfg)
    return _pack_named("LiftFeat", "the restated", liftfeat_tensor_names(cfg), liftfeat_tensor_shapes(cfg), sd, lib.imcui_hip_liftfeat_packed_floats(ca),
                       lib.imcui_hip_liftfeat_pack_weights, ca), cfg  # fmt: skip


def liftfeat_check_args(image_shape) -> None:
    """Refused before anything is launched: the reference's wrapper runs `squeeze().transpose(1, 2, 0)` (liftfeat.py:35-36), which fails on
    a gray image."""
    if len(image_shape) != 4 or image_shape[1] != 3:
        raise ValueError(f"LiftFeat expects an RGB image [B,3,H,W] (the wrapper's transpose(1, 2, 0) needs three channels), got shape {tuple(image_shape)}")


def liftfeat_pad(v: int) -> int:
    return (v + 31) // 32 * 32


class LiftFeatHIP:
    def __init__(self, cfg: dict):
        self.cfg = cfg
        self._ca = liftfeat_cfg_array(cfg)
        self._ws = _Workspace()

    def forward(self, packed: torch.Tensor, image: torch.Tensor, conf: dict, want_dense: bool = False, kcap: int | None = None):
        """image [B,3,H,W] float32 in [0,1] on the GPU -> fixed-stride outputs, no host synchronisation: keypoints [B,K,2], scores [B,K],
        descriptors [B,K,64], num_keypoints [B] int32, status [1] int32 (bit 1: `kcap` too small); with `want_dense` also kpt_heat
        [B,Hp,Wp], normals [B,Hp/8,Wp/8,192], boosted [B,Hp/8,Wp/8,64].  Order per image: row-major when the count is at most
        `max_keypoints`, else ascending score (the last `max_keypoints`; 0 keeps all, -k drops the k lowest)."""
        liftfeat_check_args(tuple(image.shape))
        hd = get_handle(image.device)
        _same_device(packed, image)
        lib = hd.lib
        image = image.contiguous().float()
        B, Cc, H, W = image.shape
        k = int(conf["max_keypoints"])
        bound = lib.imcui_hip_liftfeat_max_keypoints_bound(H, W)
        if kcap is None:
            kcap = bound if k <= 0 else max(1, min(k, bound))
        dev = image.device
        Hp, Wp = liftfeat_pad(H), liftfeat_pad(W)
        kpts, scores, desc, nk, status, out = _sparse_outputs(B, kcap, 64, dev)
        heat = torch.empty((B, Hp, Wp), dtype=torch.float32, device=dev) if want_dense else None
        nrm = torch.empty((B, Hp // 8, Wp // 8, 192), dtype=torch.float32, device=dev) if want_dense else None
        boost = torch.empty((B, Hp // 8, Wp // 8, 64), dtype=torch.float32, device=dev) if want_dense else None
        with self._ws.use(lib.imcui_hip_liftfeat_workspace_bytes(B, H, W), dev) as ws:
            hd.launch(
                lib.imcui_hip_liftfeat_forward, self._ca, _ptr(packed), _ptr(image), B, Cc, H, W, float(conf["keypoint_threshold"]), k, kcap,
                _ptr(kpts), _ptr(scores), _ptr(desc), _ptr(nk), _ptr(status), _ptr(heat), _ptr(nrm), _ptr(boost), _ptr(ws), ws.numel(),
            )  # fmt: skip
        if want_dense:
            out.update(kpt_heat=heat, normals=nrm, boosted=boost)
        return out

    # ---- test entries
    def input_probe(self, image: torch.Tensor):
        """image [B,3,H,W] -> gray [B,Hp,Wp] (zero in the pad), norm [B,2] = (invstd, -mean * invstd) over the padded image."""
        hd = get_handle(image.device)
        image = image.contiguous().float()
        B, _, H, W = image.shape
        Hp, Wp = liftfeat_pad(H), liftfeat_pad(W)
        gray = torch.empty((B, Hp, Wp), dtype=torch.float32, device=image.device)
        norm = torch.empty((B, 2), dtype=torch.float32, device=image.device)
        with self._ws.use(B * ((Hp * Wp + 4095) // 4096) * 16, image.device) as ws:
            hd.launch(hd.lib.imcui_hip_liftfeat_input_probe, _ptr(image), B, H, W, _ptr(gray), _ptr(norm), _ptr(ws), ws.numel())
        return gray, norm

    def upconv_probe(self, packed: torch.Tensor, x: torch.Tensor, stage: int, fused: bool = False, align_corners: bool = True,
                     slope: float = LIFTFEAT_SLOPE):
        """Up-conv stage 0 / 1 / 2 on x [B,h,w,cin] (NHWC) -> [B,2h,2w,cin/2]; `fused` (stage 2) -> the unfolded unit normals
        [B,2h/8,2w/8,192]."""
        hd = get_handle(x.device)
        x = x.contiguous().float()
        B, h, w, cin = x.shape
        if cin != (64, 32, 16)[stage]:
            raise ValueError(f"stage {stage} takes {(64, 32, 16)[stage]} channels, got {cin}")
        shape = (B, 2 * h // 8, 2 * w // 8, 192) if fused else (B, 2 * h, 2 * w, cin // 2)
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
        hd.launch(hd.lib.imcui_hip_liftfeat_upconv_probe, self._ca, _ptr(packed), _ptr(x), stage, int(fused), B, h, w, int(align_corners), float(slope), _ptr(out))
        return out

    def booster_probe(self, packed: torch.Tensor, d: torch.Tensor, k: torch.Tensor, n: torch.Tensor):
        """d [B,N,64], k [B,N,65], n [B,N,192] -> (out [B,N,64] unit rows, x_enc [B,N,64] the encoders' sum)."""
        hd = get_handle(d.device)
        d, k, n = d.contiguous().float(), k.contiguous().float(), n.contiguous().float()
        B, N, _ = d.shape
        out, xe = torch.empty_like(d), torch.empty_like(d)
        with self._ws.use(hd.lib.imcui_hip_liftfeat_tokens_workspace_bytes(B, N), d.device) as ws:
            hd.launch(hd.lib.imcui_hip_liftfeat_booster_probe, self._ca, _ptr(packed), _ptr(d), _ptr(k), _ptr(n), B, N, _ptr(out), _ptr(xe), _ptr(ws), ws.numel())
        return out, xe

    def aft_probe(self, packed: torch.Tensor, x: torch.Tensor, layer: int):
        """AFT layer `layer` on x [B,N,64] -> (out [B,N,64], kv [B,64])."""
        hd = get_handle(x.device)
        x = x.contiguous().float()
        B, N, _ = x.shape
        out = torch.empty_like(x)
        kv = torch.empty((B, 64), dtype=torch.float32, device=x.device)
        with self._ws.use(hd.lib.imcui_hip_liftfeat_tokens_workspace_bytes(B, N), x.device) as ws:
            hd.launch(hd.lib.imcui_hip_liftfeat_aft_probe, self._ca, _ptr(packed), _ptr(x), int(layer), B, N, _ptr(out), _ptr(kv), _ptr(ws), ws.numel())
        return out, kv

    def select_probe(self, heat: torch.Tensor, boosted: torch.Tensor, H: int, W: int, threshold: float, max_keypoints: int, kcap: int | None = None):
        """The selection on heat [B,Hp,Wp] and boosted [B,Hp/8,Wp/8,64] for images of H x W -> the outputs of `forward`."""
        hd = get_handle(heat.device)
        heat, boosted = heat.contiguous().float(), boosted.contiguous().float()
        B, Hp, Wp = heat.shape
        if kcap is None:
            bound = ((Hp + 2) // 3) * ((Wp + 2) // 3)
            kcap = bound if max_keypoints <= 0 else max(1, min(max_keypoints, bound))
        kpts, scores, desc, nk, status, out = _sparse_outputs(B, kcap, 64, heat.device)
        with self._ws.use(hd.lib.imcui_hip_liftfeat_select_workspace_bytes(B, Hp, Wp), heat.device) as ws:
            hd.launch(hd.lib.imcui_hip_liftfeat_select_probe, _ptr(heat), _ptr(boosted), B, int(H), int(W), Hp, Wp, float(threshold), int(max_keypoints), kcap,
                      _ptr(kpts), _ptr(scores), _ptr(desc), _ptr(nk), _ptr(status), _ptr(ws), ws.numel())  # fmt: skip
        return out


# ------------------------------------------------------------------ ALIKED
ALIKED_MODELS = ("aliked-n16", "aliked-n16rot")  # (c1,c2,c3,c4,dim,K,M) = (16,32,64,128,128,3,16): what csrc/aliked.hip is built for


def aliked_tensor_names() -> list[str]:
    lib = load_library()
    return [lib.imcui_hip_aliked_tensor_name(i).decode() for i in range(lib.imcui_hip_aliked_num_tensors())]


def aliked_tensor_shapes() -> dict:
    """Upstream ALIKED's state-dict shapes for aliked-n16 (without the `num_batches_tracked` counters)."""
    ch = [3, 16, 32, 64, 128]
    shapes = {}
    for b in range(1, 5):
        cin, cout = ch[b - 1], ch[b]
        for j in (1, 2):
            ci = cin if j == 1 else cout
            if b >= 3:
                shapes[f"block{b}.conv{j}.offset_conv.weight"] = (18, ci, 3, 3)
                shapes[f"block{b}.conv{j}.offset_conv.bias"] = (18,)
                shapes[f"block{b}.conv{j}.regular_conv.weight"] = (cout, ci, 3, 3)
            else:
                shapes[f"block{b}.conv{j}.weight"] = (cout, ci, 3, 3)
            for k in ("weight", "bias", "running_mean", "running_var"):
                shapes[f"block{b}.bn{j}.{k}"] = (cout,)
        if b >= 2:
            shapes[f"block{b}.downsample.weight"] = (cout, cin, 1, 1)
    for i in range(1, 5):
        shapes[f"conv{i}.weight"] = (32, ch[i], 1, 1)
    shapes.update({"score_head.0.weight": (8, 128, 1, 1), "score_head.2.weight": (4, 8, 3, 3), "score_head.4.weight": (4, 4, 3, 3),
                   "score_head.6.weight": (1, 4, 3, 3), "desc_head.agg_weights": (16, 128, 128), "desc_head.offset_conv.0.weight": (32, 128, 3, 3),
                   "desc_head.offset_conv.0.bias": (32,), "desc_head.offset_conv.2.weight": (32, 32, 1, 1), "desc_head.offset_conv.2.bias": (32,),
                   "desc_head.sf_conv.weight": (128, 128, 1, 1)})  # fmt: skip
    return shapes


def aliked_check_model(model_name: str) -> None:
    if model_name not in ALIKED_MODELS:
        known = "aliked-t16 / aliked-n32 have other channel counts and sample numbers" if model_name in ("aliked-t16", "aliked-n32") else "unknown name"
        raise ImcuiHipError(f"ALIKED model '{model_name}' is not served by the HIP backend ({known}); supported: {', '.join(ALIKED_MODELS)}")


def pack_aliked(state_dict: dict, model_name: str = "aliked-n16") -> torch.Tensor:
    """Upstream ALIKED state dict -> packed float32 buffer (host); BatchNorm (eval) is folded into the convolutions by the packer.
    Strict: `num_batches_tracked` counters are ignored, every other key is consumed exactly once, every shape checked."""
    aliked_check_model(model_name)
    lib = load_library()
    sd = {k: v for k, v in state_dict.items() if not k.endswith("num_batches_tracked")}
    return _pack_named("ALIKED", f"upstream's {model_name}", aliked_tensor_names(), aliked_tensor_shapes(), sd, lib.imcui_hip_aliked_packed_floats(),
                       lib.imcui_hip_aliked_pack_weights)


def aliked_check_args(image_shape, nms_radius: int) -> None:
    """Refusals raised before anything is launched."""
    if len(image_shape) != 4 or image_shape[1] != 3:
        raise ValueError(f"ALIKED expects an RGB image [B,3,H,W], got shape {tuple(image_shape)}")
    if not 1 <= int(nms_radius) <= 4:
        raise ValueError(f"nms_radius={nms_radius} is outside what the NMS kernel serves (1..4)")
    if image_shape[2] < 32 or image_shape[3] < 32:
        raise ValueError(f"ALIKED needs images of at least 32 x 32, got {tuple(image_shape[2:])}")


class AlikedHIP:
    N_LIMIT_MAX = 20000  # upstream's n_limit_max

    def __init__(self):
        self._ws = _Workspace()

    def forward(self, packed: torch.Tensor, image: torch.Tensor, conf: dict, want_maps: bool = False, kcap: int | None = None):
        """image [B,3,H,W] float32 on the GPU -> fixed-stride outputs, no host synchronisation: keypoints [B,K,2] (refined pixels,
        row-major order of their integer candidates), scores [B,K], descriptors [B,K,128], num_keypoints [B] int32, status [1] int32
        (bit 1: `kcap` too small).  want_maps adds score_map [B,H,W], keypoints_norm [B,K,2] and the outputs of the two deformable
        blocks x3 [B,Hp/8,Wp/8,64], x4 [B,Hp/32,Wp/32,128].  K = min(n_limit, the NMS bound)."""
        r = int(conf["nms_radius"])
        aliked_check_args(tuple(image.shape), r)
        hd = get_handle(image.device)
        _same_device(packed, image)
        lib = hd.lib
        image = image.contiguous().float()
        B, _, H, W = image.shape
        maxk = int(conf["max_num_keypoints"])
        limit = maxk if maxk > 0 else self.N_LIMIT_MAX
        if kcap is None:
            kcap = max(1, min(limit, lib.imcui_hip_aliked_max_keypoints_bound(H, W, r)))
        dev = image.device
        f32 = dict(dtype=torch.float32, device=dev)
        kpts, scores, desc, nk, status, out = _sparse_outputs(B, kcap, 128, dev)
        Hp, Wp = (H + 31) // 32 * 32, (W + 31) // 32 * 32
        smap = torch.empty((B, H, W), **f32) if want_maps else None
        kn = torch.empty((B, kcap, 2), **f32) if want_maps else None
        x3 = torch.empty((B, Hp // 8, Wp // 8, 64), **f32) if want_maps else None
        x4 = torch.empty((B, Hp // 32, Wp // 32, 128), **f32) if want_maps else None
        with self._ws.use(lib.imcui_hip_aliked_workspace_bytes(B, H, W), dev) as ws:
            hd.launch(
                lib.imcui_hip_aliked_forward, _ptr(packed), _ptr(image), B, H, W, r, float(conf["detection_threshold"]), maxk, kcap,
                _ptr(kpts), _ptr(scores), _ptr(desc), _ptr(nk), _ptr(status), _ptr(smap), _ptr(kn), _ptr(x3), _ptr(x4), _ptr(ws), ws.numel(),
            )  # fmt: skip
        if want_maps:
            out.update(score_map=smap, keypoints_norm=kn, x3=x3, x4=x4)
        return out


# ------------------------------------------------------------------ ALIKE
ALIKE_MODELS = {"alike-t": 0, "alike-s": 1, "alike-n": 2}  # the variant numbers of include/imcui_hip.h
ALIKE_CFG = {"alike-t": (8, 16, 32, 64, 64), "alike-s": (8, 16, 48, 96, 96), "alike-n": (16, 32, 64, 128, 128)}  # (c1, c2, c3, c4, dim)


def alike_check_model(model_name: str) -> int:
    """The variant number of a served model; alike-l and unknown names are refused by name."""
    if model_name not in ALIKE_MODELS:
        known = "alike-l has a second head layer (convhead1 + ReLU) that the sparse head cannot express" if model_name == "alike-l" else "unknown name"
        raise ImcuiHipError(f"ALIKE model '{model_name}' is not served by the HIP backend ({known}); supported: {', '.join(ALIKE_MODELS)}")
    return ALIKE_MODELS[model_name]


def alike_tensor_names(model_name: str = "alike-t") -> list[str]:
    v, lib = alike_check_model(model_name), load_library()
    return [lib.imcui_hip_alike_tensor_name(v, i).decode() for i in range(lib.imcui_hip_alike_num_tensors(v))]


def alike_tensor_shapes(model_name: str = "alike-t") -> dict:
    """Upstream ALIKE's state-dict shapes (without the `num_batches_tracked` counters)."""
    alike_check_model(model_name)
    c1, c2, c3, c4, dim = ALIKE_CFG[model_name]
    ch = [3, c1, c2, c3, c4]
    shapes = {}
    for b in range(1, 5):
        cin, cout = ch[b - 1], ch[b]
        for j in (1, 2):
            shapes[f"block{b}.conv{j}.weight"] = (cout, cin if j == 1 else cout, 3, 3)
            for k in ("weight", "bias", "running_mean", "running_var"):
                shapes[f"block{b}.bn{j}.{k}"] = (cout,)
        if b >= 2:
            shapes[f"block{b}.downsample.weight"] = (cout, cin, 1, 1)
            shapes[f"block{b}.downsample.bias"] = (cout,)
    for i in range(1, 5):
        shapes[f"conv{i}.weight"] = (dim // 4, ch[i], 1, 1)
    shapes["convhead2.weight"] = (dim + 1, dim, 1, 1)
    return shapes


def pack_alike(state_dict: dict, model_name: str = "alike-t") -> torch.Tensor:
    """Upstream ALIKE state dict -> packed float32 buffer (host); BatchNorm (eval) is folded into the convolutions by the packer.
    Strict: `num_batches_tracked` counters are ignored, every other key is consumed exactly once, every shape checked."""
    v = alike_check_model(model_name)
    lib = load_library()
    sd = {k: t for k, t in state_dict.items() if not k.endswith("num_batches_tracked")}
    return _pack_named("ALIKE", f"upstream's {model_name}", alike_tensor_names(model_name), alike_tensor_shapes(model_name), sd,
                       lib.imcui_hip_alike_packed_floats(v), lib.imcui_hip_alike_pack_weights, v)


def alike_check_args(image_shape, model_name: str = "alike-t") -> None:
    """Refusals raised before anything is launched."""
    alike_check_model(model_name)
    if len(image_shape) != 4 or image_shape[1] != 3:  # (the reference fails its `three == 3` assertion on gray input)
        raise ValueError(f"ALIKE expects an RGB image [B,3,H,W], got shape {tuple(image_shape)}")
    if image_shape[2] < 32 or image_shape[3] < 32:
        raise ValueError(f"ALIKE needs images of at least 32 x 32, got {tuple(image_shape[2:])}")


class AlikeHIP:
    def __init__(self, model_name: str = "alike-t"):
        self.variant = alike_check_model(model_name)
        self.model_name = model_name
        self.dims = ALIKE_CFG[model_name]
        self._ws = _Workspace()

    def forward(self, packed: torch.Tensor, image: torch.Tensor, conf: dict, want_maps: bool = False, kcap: int | None = None):
        """image [B,3,H,W] float32 on the GPU -> fixed-stride outputs, no host synchronisation: keypoints [B,K,2] (pixels), scores [B,K],
        descriptors [B,K,dim], num_keypoints [B] int32, status [1] int32 (bit 1: `kcap` too small).  Order: row-major, or descending score
        for the top_k route and after an n_limit cut.  want_maps adds score_map [B,H,W], x4 [B,Hp/32,Wp/32,c4 stored] and the branch maps
        f2 / f3 / f4 [B,Hp/2^s,Wp/2^s,dim/4].  K = min(top_k, n_limit, the NMS bound)."""
        alike_check_args(tuple(image.shape), self.model_name)
        hd = get_handle(image.device)
        _same_device(packed, image)
        lib, v = hd.lib, self.variant
        image = image.contiguous().float()
        B, _, H, W = image.shape
        top_k, n_limit = int(conf["top_k"]), int(conf["max_keypoints"])
        dim = self.dims[4]
        if kcap is None:
            kcap = lib.imcui_hip_alike_max_keypoints_bound(H, W)
            for lim in (top_k, n_limit):
                if lim > 0:
                    kcap = min(kcap, lim)
        kcap = max(1, min(int(kcap), H * W))
        dev = image.device
        f32 = dict(dtype=torch.float32, device=dev)
        kpts, scores, desc, nk, status, out = _sparse_outputs(B, kcap, dim, dev)
        Hp, Wp = (H + 31) // 32 * 32, (W + 31) // 32 * 32
        maps = {}
        if want_maps:
            c4p = (self.dims[3] + 31) // 32 * 32
            maps = dict(score_map=torch.empty((B, H, W), **f32), x4=torch.empty((B, Hp // 32, Wp // 32, c4p), **f32),
                        f2=torch.empty((B, Hp // 2, Wp // 2, dim // 4), **f32), f3=torch.empty((B, Hp // 8, Wp // 8, dim // 4), **f32),
                        f4=torch.empty((B, Hp // 32, Wp // 32, dim // 4), **f32))  # fmt: skip
        with self._ws.use(lib.imcui_hip_alike_workspace_bytes(v, B, H, W), dev) as ws:
            hd.launch(
                lib.imcui_hip_alike_forward, v, _ptr(packed), _ptr(image), B, H, W, float(conf["detection_threshold"]), top_k, n_limit,
                int(bool(conf.get("sub_pixel", False))), kcap, _ptr(kpts), _ptr(scores), _ptr(desc), _ptr(nk), _ptr(status), _ptr(maps.get("score_map")),
                _ptr(maps.get("x4")), _ptr(maps.get("f2")), _ptr(maps.get("f3")), _ptr(maps.get("f4")), _ptr(ws), ws.numel(),
            )  # fmt: skip
        out.update(maps)
        return out

    def desc_probe(self, packed: torch.Tensor, image: torch.Tensor, xy: torch.Tensor) -> torch.Tensor:
        """Test entry: the sparse descriptor head at integer pixels xy [n,2] (x, y) of ONE image [1,3,H,W] -> [n,dim]."""
        alike_check_args(tuple(image.shape), self.model_name)
        hd = get_handle(image.device)
        lib, v = hd.lib, self.variant
        image = image.contiguous().float()
        _, _, H, W = image.shape
        xy = xy.to(device=image.device, dtype=torch.int32).contiguous()
        n = xy.shape[0]
        if n == 0 or int(xy[:, 0].min()) < 0 or int(xy[:, 0].max()) >= W or int(xy[:, 1].min()) < 0 or int(xy[:, 1].max()) >= H:
            raise ValueError("desc_probe: pixels outside the image (or none)")
        desc = torch.empty((n, self.dims[4]), dtype=torch.float32, device=image.device)
        with self._ws.use(lib.imcui_hip_alike_workspace_bytes(v, 1, H, W), image.device) as ws:
            hd.launch(lib.imcui_hip_alike_desc_probe, v, _ptr(packed), _ptr(image[:1]), H, W, _ptr(xy), n, _ptr(desc), _ptr(ws), ws.numel())
        return desc


# ------------------------------------------------------------------ R2D2
# (cin, cout, kernel, conv index in upstream's flat `ops` list, BatchNorm behind it): Quad_L2Net_ConfCFS, csrc/r2d2.hip
R2D2_LAYERS = ((3, 32, 3, 0, True), (32, 32, 3, 3, True), (32, 64, 3, 6, True), (64, 64, 3, 9, True), (64, 128, 3, 12, True),
               (128, 128, 3, 15, True), (128, 128, 2, 18, True), (128, 128, 2, 20, True), (128, 128, 2, 22, False))  # fmt: skip
R2D2_NET = "Quad_L2Net_ConfCFS"
R2D2_MAX_LEVELS = 32


def r2d2_tensor_names() -> list[str]:
    lib = load_library()
    return [lib.imcui_hip_r2d2_tensor_name(i).decode() for i in range(lib.imcui_hip_r2d2_num_tensors())]


def r2d2_tensor_shapes() -> dict:
    shapes = {}
    for cin, cout, k, op, bn in R2D2_LAYERS:
        shapes[f"ops.{op}.weight"] = (cout, cin, k, k)
        shapes[f"ops.{op}.bias"] = (cout,)
        if bn:
            shapes[f"ops.{op + 1}.running_mean"] = (cout,)
            shapes[f"ops.{op + 1}.running_var"] = (cout,)
    shapes.update({"clf.weight": (2, 128, 1, 1), "clf.bias": (2,), "sal.weight": (1, 128, 1, 1), "sal.bias": (1,)})
    return shapes


def r2d2_unwrap(checkpoint: dict) -> dict:
    """Upstream's checkpoint {'net': 'Quad_L2Net_ConfCFS()', 'state_dict': ...} (or a bare state dict) -> state dict without the
    `module.` prefix.  A 'net' string that names another class (Fast_Quad_L2Net_ConfCFS: faster2d2) is refused by name."""
    sd = checkpoint
    if isinstance(checkpoint, dict) and "state_dict" in checkpoint:
        net = str(checkpoint.get("net", R2D2_NET + "()"))
        if net.split("(")[0].strip() != R2D2_NET:
            raise ImcuiHipError(f"R2D2 checkpoint builds '{net}': only {R2D2_NET} (r2d2_WASF_N16 / r2d2_WASF_N8 / r2d2_WAF_N16) is served by the "
                                "HIP backend; faster2d2 (Fast_Quad_L2Net_ConfCFS) has other layers")  # fmt: skip
        sd = checkpoint["state_dict"]
    return {(k[len("module."):] if k.startswith("module.") else k): v for k, v in sd.items()}


def pack_r2d2(state_dict: dict) -> torch.Tensor:
    """R2D2 checkpoint or state dict -> packed float32 buffer (host); the affine-free BatchNorms (eval) are folded into the convolutions.
    Strict: `num_batches_tracked` counters are ignored, every other key is consumed exactly once, every shape checked."""
    lib = load_library()
    sd = {k: t for k, t in r2d2_unwrap(state_dict).items() if not k.endswith("num_batches_tracked")}
    return _pack_named("R2D2", f"upstream's {R2D2_NET}", r2d2_tensor_names(), r2d2_tensor_shapes(), sd, lib.imcui_hip_r2d2_packed_floats(),
                       lib.imcui_hip_r2d2_pack_weights)


def r2d2_levels(H: int, W: int, scale_f: float = 2**0.25, min_size: int = 256, max_size: int = 1024, min_scale: float = 0, max_scale: float = 1) -> list:
    """extract_multiscale's schedule (naver/r2d2 extract.py), upstream's own float64 arithmetic and banker's `round`:
    [(nh, nw, runs)] from the full image down; level l + 1 is interpolated from level l whether or not level l runs."""
    if max_scale > 1:
        raise ValueError(f"R2D2: max_scale={max_scale} above 1 (upstream asserts max_scale <= 1: would blur the image)")
    if not scale_f > 1:
        raise ValueError(f"R2D2: scale_factor={scale_f} must be above 1")
    levels = []
    s = 1.0
    nh, nw = H, W
    while s + 0.001 >= max(min_scale, min_size / max(H, W)):
        levels.append((nh, nw, s - 0.001 <= min(max_scale, max_size / max(H, W))))
        s /= scale_f
        nh, nw = round(H * s), round(W * s)
        if nh < 1 or nw < 1:  # (upstream's interpolate raises on an empty size)
            break
    while levels and not levels[-1][2]:  # trailing levels that do not run are never needed
        levels.pop()
    return levels


def r2d2_check_args(image_shape, conf: dict) -> list:
    """Refusals raised before anything is launched; returns the level list."""
    if len(image_shape) != 4 or image_shape[1] != 3:
        raise ValueError(f"R2D2 expects an RGB image [B,3,H,W], got shape {tuple(image_shape)}")
    H, W = int(image_shape[2]), int(image_shape[3])
    lv = r2d2_levels(H, W, conf["scale_factor"], conf["min_size"], conf["max_size"], conf["min_scale"], conf["max_scale"])
    if len(lv) > R2D2_MAX_LEVELS:
        raise ValueError(f"R2D2: {len(lv)} pyramid levels for {H}x{W} (at most {R2D2_MAX_LEVELS}: raise scale_factor or min_size)")
    return lv


class R2D2HIP:
    def __init__(self):
        self._ws = _Workspace()

    @staticmethod
    def _arrays(levels):
        n = len(levels)
        nh = (C.c_int * n)(*[l[0] for l in levels])
        nw = (C.c_int * n)(*[l[1] for l in levels])
        run = (C.c_int * n)(*[int(l[2]) for l in levels])
        return n, nh, nw, run

    def forward(self, packed: torch.Tensor, image: torch.Tensor, conf: dict, want_maps: bool = False, kcap: int | None = None):
        """image [B,3,H,W] float32 RGB in [0,1] on the GPU -> fixed-stride outputs, no host synchronisation: keypoints [B,K,2] (pixels of
        the input image), scores [B,K], descriptors [B,K,128], num_keypoints [B] int32, status [1] int32 (bit 1: more candidates than
        `kcap`), rows in ascending score order.  K = max_keypoints, or kcap when max_keypoints is 0 (all).  kcap defaults to the bound
        for maps without exact ties (3x3 maxima are not adjacent); "all" = every pixel of every level that runs.
        want_maps adds `levels` and per running level reliability / repeatability [B,nh,nw] and the final map [B,nh,nw,128] as lists."""
        levels = r2d2_check_args(tuple(image.shape), conf)
        hd = get_handle(image.device)
        _same_device(packed, image)
        lib = hd.lib
        image = image.contiguous().float()
        B, _, H, W = image.shape
        dev = image.device
        running = [l for l in levels if l[2]]
        npix_run = sum(l[0] * l[1] for l in running)
        if kcap is None:
            kcap = sum(((l[0] + 1) // 2) * ((l[1] + 1) // 2) for l in running)
        elif kcap == "all":
            kcap = npix_run
        kcap = max(1, min(int(kcap), npix_run))
        maxk = int(conf["max_keypoints"] or 0)
        kout = kcap if maxk <= 0 else min(maxk, kcap)
        kpts, scores, desc, nk, status, out = _sparse_outputs(B, kout, 128, dev)
        n, nh, nw, run = self._arrays(levels)
        maps = {}
        if want_maps:
            f32 = dict(dtype=torch.float32, device=dev)
            maps = dict(rel=torch.empty(B * npix_run, **f32), rep=torch.empty(B * npix_run, **f32), fmap=torch.empty(B * npix_run * 128, **f32))
        if n == 0 or not running:  # (min_size above the image and max_size below it: upstream returns nothing)
            for t in (kpts, scores, desc, nk, status):
                t.zero_()
            return out
        with self._ws.use(lib.imcui_hip_r2d2_workspace_bytes(B, n, nh, nw, kcap), dev) as ws:
            hd.launch(
                lib.imcui_hip_r2d2_forward, _ptr(packed), _ptr(image), B, H, W, n, nh, nw, run, float(conf["reliability_threshold"]),
                float(conf["repetability_threshold"]), maxk, kcap, kout, _ptr(kpts), _ptr(scores), _ptr(desc), _ptr(nk), _ptr(status),
                _ptr(maps.get("rel")), _ptr(maps.get("rep")), _ptr(maps.get("fmap")), _ptr(ws), ws.numel(),
            )  # fmt: skip
        if want_maps:
            out["levels"] = [(l[0], l[1]) for l in running]
            out["reliability"], out["repeatability"], out["final_map"] = [], [], []
            off = 0
            for lh, lw, _ in running:
                m = B * lh * lw
                out["reliability"].append(maps["rel"][off : off + m].view(B, lh, lw))
                out["repeatability"].append(maps["rep"][off : off + m].view(B, lh, lw))
                out["final_map"].append(maps["fmap"][off * 128 : (off + m) * 128].view(B, lh, lw, 128))
                off += m
        return out

    def desc_probe(self, packed: torch.Tensor, image: torch.Tensor, xy: torch.Tensor) -> torch.Tensor:
        """Test entry: F.normalize of the network's final map at integer pixels xy [n,2] (x, y) of ONE image [1,3,H,W] -> [n,128]."""
        if image.dim() != 4 or image.shape[1] != 3:
            raise ValueError(f"R2D2 expects an RGB image [B,3,H,W], got shape {tuple(image.shape)}")
        hd = get_handle(image.device)
        lib = hd.lib
        image = image.contiguous().float()
        _, _, H, W = image.shape
        xy = xy.to(device=image.device, dtype=torch.int32).contiguous()
        n = xy.shape[0]
        if n == 0 or int(xy[:, 0].min()) < 0 or int(xy[:, 0].max()) >= W or int(xy[:, 1].min()) < 0 or int(xy[:, 1].max()) >= H:
            raise ValueError("desc_probe: pixels outside the image (or none)")
        desc = torch.empty((n, 128), dtype=torch.float32, device=image.device)
        nh, nw = (C.c_int * 1)(H), (C.c_int * 1)(W)
        with self._ws.use(lib.imcui_hip_r2d2_workspace_bytes(1, 1, nh, nw, 1), image.device) as ws:
            hd.launch(lib.imcui_hip_r2d2_desc_probe, _ptr(packed), _ptr(image[:1]), H, W, _ptr(xy), n, _ptr(desc), _ptr(ws), ws.numel())
        return desc


# ------------------------------------------------------------------ D2-Net / RoRD
# (cin, cout, dilation, index in DenseFeatureExtractionModule.model): VGG-16 cut at conv4_3, csrc/d2net.hip
D2NET_LAYERS = ((3, 64, 1, 0), (64, 64, 1, 2), (64, 128, 1, 5), (128, 128, 1, 7), (128, 256, 1, 10), (256, 256, 1, 12), (256, 256, 1, 14),
                (256, 512, 2, 17), (512, 512, 2, 19), (512, 512, 2, 21))  # fmt: skip
D2NET_SCALES_SS, D2NET_SCALES_MS = (1,), (0.5, 1, 2)  # process_multiscale: `scales=[1]` (d2net.py:46) and its default
D2NET_MAX_LEVELS = 8


def d2net_tensor_names() -> list[str]:
    lib = load_library()
    return [lib.imcui_hip_d2net_tensor_name(i).decode() for i in range(lib.imcui_hip_d2net_num_tensors())]


def d2net_tensor_shapes() -> dict:
    shapes = {}
    for cin, cout, _, op in D2NET_LAYERS:
        shapes[f"dense_feature_extraction.model.{op}.weight"] = (cout, cin, 3, 3)
        shapes[f"dense_feature_extraction.model.{op}.bias"] = (cout,)
    return shapes


def pack_d2net(state_dict: dict) -> torch.Tensor:
    """D2-Net / RoRD checkpoint ({'model': state dict}, as lib/model_test.py loads it) or a bare state dict -> packed float32 buffer
    (host).  Strict: every key is consumed exactly once, every shape checked."""
    lib = load_library()
    sd = state_dict
    if isinstance(sd, dict) and "model" in sd and isinstance(sd["model"], dict):
        sd = sd["model"]
    return _pack_named("D2-Net", "upstream's DenseFeatureExtractionModule", d2net_tensor_names(), d2net_tensor_shapes(), dict(sd),
                       lib.imcui_hip_d2net_packed_floats(), lib.imcui_hip_d2net_pack_weights)


def d2net_levels(H: int, W: int, scales=D2NET_SCALES_SS) -> list:
    """process_multiscale's level images: F.interpolate(scale_factor=s) gives floor(H * s) x floor(W * s), evaluated in float64 as ATen
    does; in list order.  A level whose feature map (size // 4 - 1) would be empty is refused."""
    if not 1 <= len(scales) <= D2NET_MAX_LEVELS:
        raise ValueError(f"D2-Net: {len(scales)} scales (1..{D2NET_MAX_LEVELS})")
    levels = []
    for s in scales:
        lh, lw = int(math.floor(float(H) * float(s))), int(math.floor(float(W) * float(s)))
        if lh // 4 - 1 < 1 or lw // 4 - 1 < 1:
            raise ValueError(f"D2-Net: the {H}x{W} image at scale {s} is {lh}x{lw}, its feature map ({lh // 4 - 1}x{lw // 4 - 1}) is empty: "
                             "every level needs at least 8x8 pixels")  # fmt: skip
        levels.append((lh, lw))
    return levels


def d2net_check_args(image_shape, scales=D2NET_SCALES_SS) -> list:
    """Refusals raised before anything is launched; returns the level list."""
    if len(image_shape) != 4 or image_shape[1] != 3:
        raise ValueError(f"D2-Net expects an RGB image [B,3,H,W], got shape {tuple(image_shape)}")
    return d2net_levels(int(image_shape[2]), int(image_shape[3]), scales)


class D2NetHIP:
    def __init__(self):
        self._ws = _Workspace()

    def forward(self, packed: torch.Tensor, image: torch.Tensor, conf: dict, want_maps: bool = False, kcap: int | None = None, scales=None):
        """image [B,3,H,W] float32 RGB in [0,1] on the GPU -> fixed-stride outputs, no host synchronisation: keypoints [B,K,2] (x, y in
        pixels of the input image), scores [B,K], descriptors [B,K,512], num_keypoints [B] int32, status [1] int32 (bit 1: more
        candidates than `kcap`), rows in ascending score order.  K = max_keypoints, or kcap when max_keypoints is 0 (all).  kcap
        defaults to the sum of the levels' feature-map pixels: one candidate per pixel, enough unless channels tie for the maximum.
        want_maps adds `levels` (feature-map sizes) and `dense_features`, per level [B,h,w,512] after the multi-scale sum."""
        if scales is None:
            scales = D2NET_SCALES_MS if conf.get("multiscale") else D2NET_SCALES_SS
        levels = d2net_check_args(tuple(image.shape), scales)
        hd = get_handle(image.device)
        _same_device(packed, image)
        lib = hd.lib
        image = image.contiguous().float()
        B, _, H, W = image.shape
        dev = image.device
        fsz = [(lh // 4 - 1, lw // 4 - 1) for lh, lw in levels]
        npix = sum(a * b for a, b in fsz)
        kcap = max(1, int(npix if kcap is None else kcap))
        maxk = int(conf["max_keypoints"] or 0)
        kout = kcap if maxk <= 0 else min(maxk, kcap)
        kpts, scores, desc, nk, status, out = _sparse_outputs(B, kout, 512, dev)
        n = len(levels)
        lh = (C.c_int * n)(*[l[0] for l in levels])
        lw = (C.c_int * n)(*[l[1] for l in levels])
        fmap = torch.empty(B * npix * 512, dtype=torch.float32, device=dev) if want_maps else None
        with self._ws.use(lib.imcui_hip_d2net_workspace_bytes(B, n, lh, lw, kcap), dev) as ws:
            hd.launch(
                lib.imcui_hip_d2net_forward, _ptr(packed), _ptr(image), B, H, W, n, lh, lw, int(bool(conf.get("use_relu", True))), maxk, kcap, kout,
                _ptr(kpts), _ptr(scores), _ptr(desc), _ptr(nk), _ptr(status), _ptr(fmap), _ptr(ws), ws.numel(),
            )  # fmt: skip
        if want_maps:
            out["levels"] = fsz
            out["dense_features"] = []
            off = 0
            for fh, fw in fsz:
                m = B * fh * fw * 512
                out["dense_features"].append(fmap[off : off + m].view(B, fh, fw, 512))
                off += m
        return out

    @staticmethod
    def layer_probe(op: str, inp: torch.Tensor, packed: torch.Tensor | None = None) -> torch.Tensor:
        """Test entry: one small kernel of the trunk alone.  "conv0": image [B,3,H,W] -> [B,H,W,64] (needs `packed`); "maxpool": NHWC
        [B,H,W,C] -> [B,H//2,W//2,C]; "avgpool": -> [B,H-1,W-1,C]."""
        code = {"conv0": 0, "maxpool": 1, "avgpool": 2}[op]
        hd = get_handle(inp.device)
        inp = inp.contiguous().float()
        if code == 0:
            B, _, H, W = inp.shape
            Cc, shape = 64, (B, H, W, 64)
        else:
            B, H, W, Cc = inp.shape
            shape = (B, H // 2, W // 2, Cc) if code == 1 else (B, H - 1, W - 1, Cc)
        out = torch.empty(shape, dtype=torch.float32, device=inp.device)
        hd.launch(hd.lib.imcui_hip_d2net_layer_probe, code, _ptr(packed), _ptr(inp), B, H, W, Cc, _ptr(out))
        return out

    def detect_probe(self, feat: torch.Tensor, max_keypoints: int = 0, kcap: int | None = None):
        """Test entry: detector, localization, candidate list, cut and descriptors on the caller's maps feat [B,h,w,C] (C a multiple of
        64 up to 512) as one level that is its own image -> the outputs of `forward` with descriptors [B,K,C]."""
        if feat.dim() != 4 or feat.shape[3] % 64 or not 64 <= feat.shape[3] <= 512:
            raise ValueError(f"detect_probe expects maps [B,h,w,C] with C a multiple of 64 up to 512, got {tuple(feat.shape)}")
        hd = get_handle(feat.device)
        lib = hd.lib
        feat = feat.contiguous().float()
        B, fh, fw, Cc = feat.shape
        kcap = max(1, int(fh * fw if kcap is None else kcap))
        maxk = int(max_keypoints or 0)
        kout = kcap if maxk <= 0 else min(maxk, kcap)
        kpts, scores, desc, nk, status, out = _sparse_outputs(B, kout, Cc, feat.device)
        with self._ws.use(lib.imcui_hip_d2net_probe_workspace_bytes(B, fh, fw, Cc, kcap), feat.device) as ws:
            hd.launch(lib.imcui_hip_d2net_detect_probe, _ptr(feat), B, fh, fw, Cc, maxk, kcap, kout, _ptr(kpts), _ptr(scores), _ptr(desc), _ptr(nk),
                      _ptr(status), _ptr(ws), ws.numel())  # fmt: skip
        return out


# ------------------------------------------------------------------ LANet
LANET_DIM = 256
LANET_MIN_SIDE = 8  # one 8 x 8 cell
LANET_ACTIVATIONS = {"relu": 1, "leaky_relu": 2}
LANET_LAYERS = ("1a", "1b", "2a", "2b", "3a", "3b", "4a", "4b", "Da", "Pa")  # the BatchNorm'd 3x3 layers: trunk, score / location head
_BN_KEYS = ("weight", "bias", "running_mean", "running_var")


def lanet_config(sd: dict, activation: str = "relu") -> dict:
    """What a LANet state dict (under the library's names, `lanet_tensor_names`) decides: widths, kernel size / bias / BatchNorm of the
    two level convolutions, bias on the BatchNorm'd convolutions.  Nothing is guessed: a missing key or an unexpected shape raises."""
    if activation not in LANET_ACTIVATIONS:
        raise ImcuiHipError(f"LANet: activation '{activation}' is not served ({', '.join(LANET_ACTIVATIONS)})")

    def shape(name, ndim):
        if name not in sd:
            raise ImcuiHipError(f"LANet state dict: '{name}' is missing")
        s = tuple(sd[name].shape)
        if len(s) != ndim:
            raise ImcuiHipError(f"LANet state dict: '{name}' has shape {s}, expected {ndim} dimensions")
        return s

    widths = tuple(shape(f"conv{i}b.weight", 4)[0] for i in (1, 2, 3, 4))
    for c in widths:
        if c % 32 or not 32 <= c <= 512:
            raise ImcuiHipError(f"LANet: trunk widths {widths} must be multiples of 32 (up to 512)")
    if widths[3] != LANET_DIM:
        raise ImcuiHipError(f"LANet: c4={widths[3]}, but level 4 of the descriptor is x4 itself and has to be {LANET_DIM} wide")
    ks = []
    for lvl in (2, 3):
        s = shape(f"des_conv{lvl}.weight", 4)
        if s[2] != s[3] or s[2] not in (1, 3):
            raise ImcuiHipError(f"LANet: des_conv{lvl}.weight has shape {s}: the kernel must be 1x1 or 3x3")
        ks.append(s[2])
    return {"widths": widths, "k": tuple(ks), "bias": tuple(int(f"des_conv{l}.bias" in sd) for l in (2, 3)),
            "bn": tuple(int(f"des_bn{l}.weight" in sd) for l in (2, 3)), "activation": activation, "conv_bias": int("conv1a.bias" in sd)}  # fmt: skip


def lanet_cfg_array(cfg: dict):
    """The 12 ints of include/imcui_hip.h's `cfg`."""
    return (C.c_int * 12)(*cfg["widths"], *cfg["k"], *cfg["bias"], *cfg["bn"], LANET_ACTIVATIONS[cfg["activation"]], cfg["conv_bias"])


def lanet_tensor_names(cfg: dict) -> list[str]:
    lib, ca = load_library(), lanet_cfg_array(cfg)
    return [lib.imcui_hip_lanet_tensor_name(ca, i).decode() for i in range(lib.imcui_hip_lanet_num_tensors(ca))]


def lanet_tensor_shapes(cfg: dict) -> dict:
    c1, c2, c3, c4 = cfg["widths"]
    shapes = {}
    chans = {"1a": (3, c1), "1b": (c1, c1), "2a": (c1, c2), "2b": (c2, c2), "3a": (c2, c3), "3b": (c3, c3), "4a": (c3, c4), "4b": (c4, c4),
             "Da": (c4, LANET_DIM), "Pa": (c4, LANET_DIM)}  # fmt: skip
    for name in LANET_LAYERS:
        cin, cout = chans[name]
        shapes[f"conv{name}.weight"] = (cout, cin, 3, 3)
        if cfg["conv_bias"]:
            shapes[f"conv{name}.bias"] = (cout,)
        for k in _BN_KEYS:
            shapes[f"bn{name}.{k}"] = (cout,)
    shapes["convDb.weight"], shapes["convDb.bias"] = (4, LANET_DIM, 3, 3), (4,)
    shapes["convPb.weight"], shapes["convPb.bias"] = (2, LANET_DIM, 3, 3), (2,)
    for i, (lvl, cin) in enumerate(((2, c2), (3, c3))):
        shapes[f"des_conv{lvl}.weight"] = (LANET_DIM, cin, cfg["k"][i], cfg["k"][i])
        if cfg["bias"][i]:
            shapes[f"des_conv{lvl}.bias"] = (LANET_DIM,)
        if cfg["bn"][i]:
            for k in _BN_KEYS:
                shapes[f"des_bn{lvl}.{k}"] = (LANET_DIM,)
    return shapes


def pack_lanet(state_dict: dict, activation: str = "relu"):
    """LANet state dict under the library's names (the plugin maps a checkpoint's keys) -> (packed float32 buffer (host), cfg).  BatchNorm
    (eval) is folded by the packer.  Strict: `num_batches_tracked` counters are ignored, every other key is consumed exactly once and
    every shape checked; an unknown or missing key raises."""
    lib = load_library()
    sd = {k: t for k, t in state_dict.items() if not k.endswith("num_batches_tracked")}
    cfg = lanet_config(sd, activation)
    ca = lanet_cfg_array(cfg)
    n = lib.imcui_hip_lanet_packed_floats(ca)
    if n == 0:
        raise ImcuiHipError(f"LANet: the library refuses the configuration {cfg}")
    return _pack_named("LANet", "the PointModel (network_v0)", lanet_tensor_names(cfg), lanet_tensor_shapes(cfg), sd, n, lib.imcui_hip_lanet_pack_weights, ca), cfg


def lanet_check_args(image_shape, max_keypoints: int = 0) -> None:
    """Refusals raised before anything is launched."""
    if len(image_shape) != 4 or image_shape[1] != 3:
        raise ValueError(f"LANet expects an RGB image [B,3,H,W], got shape {tuple(image_shape)}")
    if image_shape[2] < LANET_MIN_SIDE or image_shape[3] < LANET_MIN_SIDE:
        raise ValueError(f"LANet needs images of at least {LANET_MIN_SIDE} x {LANET_MIN_SIDE} (one cell), got {tuple(image_shape[2:])}")
    if int(max_keypoints) < 0:  # (the reference's slice `[-k or None:]` would silently DROP the |k| lowest scores)
        raise ValueError(f"LANet: max_keypoints={max_keypoints} is negative; 0 keeps every key-point")


class LanetHIP:
    def __init__(self, cfg: dict):
        self.cfg = cfg
        self._ca = lanet_cfg_array(cfg)
        self._ws = _Workspace()

    def forward(self, packed: torch.Tensor, image: torch.Tensor, conf: dict, want_maps: bool = False):
        """image [B,3,H,W] float32 RGB in [0,1] on the GPU -> fixed-stride outputs, no host synchronisation: keypoints [B,K,2] (x, y in
        pixels), scores [B,K], descriptors [B,K,256], num_keypoints [B] int32, status [1] int32 (always 0), rows in ascending (score,
        cell) order, rows past the count zero.  K = min(max_keypoints or all, cells).  want_maps adds x2 / x3 / x4 (NHWC) and the per-cell
        cell_score [B,Hc*Wc], cell_coord / cell_tanh [B,Hc*Wc,2], cell_aware [B,Hc*Wc,3]."""
        maxk = int(conf["max_keypoints"] or 0)
        lanet_check_args(tuple(image.shape), maxk)
        hd = get_handle(image.device)
        _same_device(packed, image)
        lib = hd.lib
        image = image.contiguous().float()
        B, _, H, W = image.shape
        dev = image.device
        np_ = (H // 8) * (W // 8)
        kout = np_ if maxk == 0 else min(maxk, np_)
        kpts, scores, desc, nk, status, out = _sparse_outputs(B, kout, LANET_DIM, dev)
        maps = {}
        if want_maps:
            f32 = dict(dtype=torch.float32, device=dev)
            c2, c3 = self.cfg["widths"][1:3]
            maps = dict(x2=torch.empty((B, H // 2, W // 2, c2), **f32), x3=torch.empty((B, H // 4, W // 4, c3), **f32),
                        x4=torch.empty((B, H // 8, W // 8, LANET_DIM), **f32), cell_score=torch.empty((B, np_), **f32),
                        cell_coord=torch.empty((B, np_, 2), **f32), cell_aware=torch.empty((B, np_, 3), **f32), cell_tanh=torch.empty((B, np_, 2), **f32))  # fmt: skip
        with self._ws.use(lib.imcui_hip_lanet_workspace_bytes(self._ca, B, H, W, kout), dev) as ws:
            hd.launch(
                lib.imcui_hip_lanet_forward, self._ca, _ptr(packed), _ptr(image), B, H, W, float(conf["keypoint_threshold"]), maxk, kout, _ptr(kpts),
                _ptr(scores), _ptr(desc), _ptr(nk), _ptr(status), _ptr(maps.get("x2")), _ptr(maps.get("x3")), _ptr(maps.get("x4")),
                _ptr(maps.get("cell_score")), _ptr(maps.get("cell_coord")), _ptr(maps.get("cell_aware")), _ptr(maps.get("cell_tanh")), _ptr(ws), ws.numel(),
            )  # fmt: skip
        out.update(maps)
        return out

    def stem_probe(self, packed: torch.Tensor, image: torch.Tensor) -> torch.Tensor:
        """Test entry: conv1a with the normalisation, image [B,3,H,W] -> [B,H,W,c1]."""
        hd = get_handle(image.device)
        image = image.contiguous().float()
        B, _, H, W = image.shape
        out = torch.empty((B, H, W, self.cfg["widths"][0]), dtype=torch.float32, device=image.device)
        scratch = torch.empty((B, H, W, 32), dtype=torch.float32, device=image.device)
        hd.launch(hd.lib.imcui_hip_lanet_stem_probe, self._ca, _ptr(packed), _ptr(image), B, H, W, _ptr(out), _ptr(scratch))
        return out

    def tail_probe(self, packed: torch.Tensor, s1: torch.Tensor, p1: torch.Tensor, H: int, W: int) -> dict:
        """Test entry: the two tails and the decode on hidden maps s1, p1 [B,Hc,Wc,256] of an H x W image."""
        hd = get_handle(s1.device)
        s1, p1 = s1.contiguous().float(), p1.contiguous().float()
        B, Hc, Wc, _ = s1.shape
        f32 = dict(dtype=torch.float32, device=s1.device)
        o = dict(cell_score=torch.empty((B, Hc * Wc), **f32), cell_coord=torch.empty((B, Hc * Wc, 2), **f32), cell_tanh=torch.empty((B, Hc * Wc, 2), **f32),
                 cell_aware=torch.empty((B, Hc * Wc, 3), **f32))  # fmt: skip
        hd.launch(hd.lib.imcui_hip_lanet_tail_probe, self._ca, _ptr(packed), _ptr(s1), _ptr(p1), B, Hc, Wc, H, W, _ptr(o["cell_score"]), _ptr(o["cell_coord"]),
                  _ptr(o["cell_tanh"]), _ptr(o["cell_aware"]))  # fmt: skip
        return o

    def select_probe(self, raw: torch.Tensor, H: int, W: int, threshold: float, max_keypoints: int = 0) -> dict:
        """Test entry: decode and selection from head outputs raw [B,Hc,Wc,6] (score head 0..3, location head 4..5) of an H x W image."""
        lanet_check_args((raw.shape[0], 3, H, W), max_keypoints)
        hd = get_handle(raw.device)
        lib = hd.lib
        raw = raw.contiguous().float()
        B, Hc, Wc, _ = raw.shape
        np_, maxk, dev = Hc * Wc, int(max_keypoints), raw.device
        kout = np_ if maxk == 0 else min(maxk, np_)
        f32 = dict(dtype=torch.float32, device=dev)
        kpts, scores, _, nk, status, out = _sparse_outputs(B, kout, 1, dev)
        out.pop("descriptors")
        o = dict(cell_score=torch.empty((B, np_), **f32), cell_coord=torch.empty((B, np_, 2), **f32), cell_aware=torch.empty((B, np_, 3), **f32),
                 cell_tanh=torch.empty((B, np_, 2), **f32))  # fmt: skip
        with self._ws.use(lib.imcui_hip_lanet_select_workspace_bytes(B, Hc, Wc, kout), dev) as ws:
            hd.launch(lib.imcui_hip_lanet_select_probe, _ptr(raw), B, Hc, Wc, H, W, float(threshold), maxk, kout, _ptr(kpts), _ptr(scores), _ptr(nk), _ptr(status),
                      _ptr(o["cell_score"]), _ptr(o["cell_coord"]), _ptr(o["cell_aware"]), _ptr(o["cell_tanh"]), _ptr(ws), ws.numel())  # fmt: skip
        out.update(o)
        return out

    def desc_probe(self, packed: torch.Tensor, x2: torch.Tensor, x3: torch.Tensor, x4: torch.Tensor, H: int, W: int, coords: torch.Tensor,
                   aware: torch.Tensor) -> torch.Tensor:
        """Test entry: the sparse descriptor head of ONE image at positions coords [n,2] (pixels of the H x W image) with level weights
        aware [n,3], from maps x2 [h2,w2,c2], x3 [h3,w3,c3], x4 [h4,w4,256] (NHWC) -> [n,256]."""
        hd = get_handle(x2.device)
        x2, x3, x4 = x2.contiguous().float(), x3.contiguous().float(), x4.contiguous().float()
        coords, aware = coords.contiguous().float(), aware.contiguous().float()
        c2, c3 = self.cfg["widths"][1:3]
        if x2.shape[-1] != c2 or x3.shape[-1] != c3 or x4.shape[-1] != LANET_DIM or coords.shape[0] != aware.shape[0] or coords.shape[0] < 1:
            raise ValueError("desc_probe: map widths or the number of positions do not match")
        n = coords.shape[0]
        desc = torch.empty((n, LANET_DIM), dtype=torch.float32, device=x2.device)
        hd.launch(hd.lib.imcui_hip_lanet_desc_probe, self._ca, _ptr(packed), _ptr(x2), x2.shape[0], x2.shape[1], _ptr(x3), x3.shape[0], x3.shape[1], _ptr(x4),
                  x4.shape[0], x4.shape[1], H, W, _ptr(coords), _ptr(aware), n, _ptr(desc))  # fmt: skip
        return desc

    def dense_levels(self, packed: torch.Tensor, x2: torch.Tensor, x3: torch.Tensor):
        """Test entry: des_conv2(x2) and des_conv3(x3) as dense maps on the shared GEMM, x2 [B,h2,w2,c2], x3 [B,h3,w3,c3] (NHWC) ->
        ([B,h2,w2,256], [B,h3,w3,256]).  The forward never runs this form."""
        hd = get_handle(x2.device)
        x2, x3 = x2.contiguous().float(), x3.contiguous().float()
        B, h2, w2, _ = x2.shape
        _, h3, w3, _ = x3.shape
        d2 = torch.empty((B, h2, w2, LANET_DIM), dtype=torch.float32, device=x2.device)
        d3 = torch.empty((B, h3, w3, LANET_DIM), dtype=torch.float32, device=x2.device)
        hd.launch(hd.lib.imcui_hip_lanet_dense_levels, self._ca, _ptr(packed), _ptr(x2), B, h2, w2, _ptr(x3), h3, w3, _ptr(d2), _ptr(d3))
        return d2, d3


# ------------------------------------------------------------------ DarkFeat
DARKFEAT_DIM = 128
DARKFEAT_MIN_SIDE = 16
DARKFEAT_STATUS_FLAT = 4  # status bit: an image of the batch is flat (std == 0)
# upstream's `det` config (THU-LYJ-Lab/DarkFeat; the reference's wrapper hands none of its conf to the network): backend-only conf keys
DARKFEAT_DET_DEFAULTS = {"score_thld": 0.5, "edge_thld": 10, "nms_size": 3, "eof_mask": 5, "kpt_n": 5000}
_DARKFEAT_DROPPED = ("running_mean", "running_var", "num_batches_tracked")  # upstream drops these before load_state_dict


def darkfeat_layers() -> list[dict]:
    """The backbone as the library's ONE table states it (csrc/darkfeat.hip, DF_LAYERS): name, cin, cout, stride, norm (InstanceNorm +
    ReLU behind the convolution), tap (the score level its raw output feeds, -1 none)."""
    lib = load_library()
    out = []
    for i in range(lib.imcui_hip_darkfeat_num_layers()):
        v = (C.c_int * 5)()
        name = lib.imcui_hip_darkfeat_layer(i, v).decode()
        out.append({"name": name, "cin": v[0], "cout": v[1], "stride": v[2], "norm": bool(v[3]), "tap": v[4]})
    return out


def darkfeat_tensor_names() -> list[str]:
    lib = load_library()
    return [lib.imcui_hip_darkfeat_tensor_name(i).decode() for i in range(lib.imcui_hip_darkfeat_num_tensors())]


def darkfeat_tensor_shapes() -> dict:
    shapes = {}
    for L in darkfeat_layers():
        shapes[f"{L['name']}.0.weight"] = (L["cout"], L["cin"], 3, 3)
        shapes[f"{L['name']}.0.bias"] = (L["cout"],)
    shapes["clf.weight"], shapes["clf.bias"] = (2, DARKFEAT_DIM, 1, 1), (2,)
    for i in range(3):
        shapes[f"moving_avg_params.{i}"] = (1,)
    return shapes


def pack_darkfeat(state_dict: dict) -> torch.Tensor:
    """DarkFeat state dict (upstream's keys: `convN.0.weight`, optional `convN.0.bias`, `clf.*`, `moving_avg_params.{0,1,2}`) -> packed
    float32 buffer (host).  Strict: the BatchNorm-statistics keys upstream drops before loading (`running_mean`, `running_var`,
    `num_batches_tracked`) are ignored, a convolution bias the checkpoint does not carry is zero, every other key is consumed exactly
    once and every shape checked; an unknown or missing key raises."""
    lib = load_library()
    sd = {k: t for k, t in state_dict.items() if not k.endswith(_DARKFEAT_DROPPED)}
    shapes = darkfeat_tensor_shapes()
    for L in darkfeat_layers():
        sd.setdefault(f"{L['name']}.0.bias", torch.zeros(L["cout"]))
    for i in range(3):  # scalars: 0-d or [1]
        k = f"moving_avg_params.{i}"
        if k in sd:
            sd[k] = torch.as_tensor(sd[k]).reshape(-1)
    n = lib.imcui_hip_darkfeat_packed_floats()
    if n == 0:
        raise ImcuiHipError("DarkFeat: the library refuses its own layer table")
    return _pack_named("DarkFeat", "the DarkFeat", darkfeat_tensor_names(), shapes, sd, n, lib.imcui_hip_darkfeat_pack_weights)


def darkfeat_map_sizes(H: int, W: int) -> tuple:
    """(h2, w2, h4, w4): a stride-2 layer leaves (n - 1) // 2 + 1 rows / columns."""
    h2, w2 = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    return h2, w2, (h2 - 1) // 2 + 1, (w2 - 1) // 2 + 1


def darkfeat_det_conf(conf: dict) -> dict:
    """The detector settings of a conf: upstream's values unless the conf carries the backend-only keys; refusals by name."""
    if conf.get("multi_scale"):
        raise ValueError("DarkFeat: multi_scale is not served by the HIP backend")
    if conf.get("multi_level", True) is False:
        raise ValueError("DarkFeat: multi_level=False is not served by the HIP backend (the score is the three-level sum)")
    if conf.get("use_peakiness", True) is False:
        raise ValueError("DarkFeat: use_peakiness=False is not served by the HIP backend")
    d = {k: conf.get(k, v) for k, v in DARKFEAT_DET_DEFAULTS.items()}
    if int(d["nms_size"]) not in (0, 3):
        raise ValueError(f"DarkFeat: nms_size={d['nms_size']} is not served (0 or 3)")
    if int(d["eof_mask"]) < 0 or int(d["kpt_n"]) < 1 or not float(d["edge_thld"]) > 0:
        raise ValueError(f"DarkFeat: eof_mask={d['eof_mask']} (>= 0), kpt_n={d['kpt_n']} (>= 1), edge_thld={d['edge_thld']} (> 0)")
    return d


def darkfeat_check_args(image_shape, max_keypoints: int = 0) -> None:
    """Refusals raised before anything is launched."""
    if len(image_shape) != 4 or image_shape[1] != 3:
        raise ValueError(f"DarkFeat expects an RGB image [B,3,H,W], got shape {tuple(image_shape)}")
    if image_shape[2] < DARKFEAT_MIN_SIDE or image_shape[3] < DARKFEAT_MIN_SIDE:
        raise ValueError(f"DarkFeat needs images of at least {DARKFEAT_MIN_SIDE} x {DARKFEAT_MIN_SIDE}, got {tuple(image_shape[2:])}")
    if int(max_keypoints) < 0:  # (the reference's slice `[-k or None:]` would silently DROP the |k| lowest scores)
        raise ValueError(f"DarkFeat: max_keypoints={max_keypoints} is negative; 0 keeps every key-point")


def _darkfeat_kout(np_: int, det: dict, maxk: int) -> int:
    return max(1, min(np_, int(det["kpt_n"]), maxk if maxk > 0 else np_))


class DarkFeatHIP:
    def __init__(self):
        self._ws = _Workspace()

    def forward(self, packed: torch.Tensor, image: torch.Tensor, conf: dict, want_maps: bool = False, layer: int = -1):
        """image [B,3,H,W] float32 on the GPU -> fixed-stride outputs, no host synchronisation: keypoints [B,K,2] (x, y in pixels,
        integer-valued), scores [B,K], descriptors [B,K,128], num_keypoints [B] int32, status [1] int32 (bit 4: a flat image), rows in
        ascending (score, pixel) order, rows past the count zero.  K = min(kpt_n, max_keypoints or all, H W).  want_maps adds score
        [B,H,W], desc_map [B,h4,w4,128], peak0 / peak1 / peak2 and prob; `layer` adds layer_raw / layer_norm of that layer (NHWC)."""
        maxk = int(conf.get("max_keypoints") or 0)
        darkfeat_check_args(tuple(image.shape), maxk)
        det = darkfeat_det_conf(conf)
        hd = get_handle(image.device)
        _same_device(packed, image)
        lib = hd.lib
        image = image.contiguous().float()
        B, Cc, H, W = image.shape
        dev = image.device
        kout = _darkfeat_kout(H * W, det, maxk)
        kpts, scores, desc, nk, status, out = _sparse_outputs(B, kout, DARKFEAT_DIM, dev)
        f32 = dict(dtype=torch.float32, device=dev)
        h2, w2, h4, w4 = darkfeat_map_sizes(H, W)
        maps = {}
        if want_maps:
            maps = dict(score=torch.empty((B, H, W), **f32), desc_map=torch.empty((B, h4, w4, DARKFEAT_DIM), **f32), peak0=torch.empty((B, H, W), **f32),
                        peak1=torch.empty((B, h2, w2), **f32), peak2=torch.empty((B, h4, w4), **f32), prob=torch.empty((B, h4, w4), **f32))  # fmt: skip
        if layer >= 0:
            sizes, hh, ww = [], H, W
            for L in darkfeat_layers():
                if L["stride"] == 2:
                    hh, ww = (hh - 1) // 2 + 1, (ww - 1) // 2 + 1
                sizes.append((B, hh, ww, L["cout"]))
            maps["layer_raw"], maps["layer_norm"] = torch.empty(sizes[layer], **f32), torch.empty(sizes[layer], **f32)
        with self._ws.use(lib.imcui_hip_darkfeat_workspace_bytes(B, H, W), dev) as ws:
            hd.launch(
                lib.imcui_hip_darkfeat_forward, _ptr(packed), _ptr(image), B, Cc, H, W, float(det["score_thld"]), float(det["edge_thld"]), int(det["nms_size"]),
                int(det["eof_mask"]), int(det["kpt_n"]), maxk, kout, _ptr(kpts), _ptr(scores), _ptr(desc), _ptr(nk), _ptr(status), _ptr(maps.get("score")),
                _ptr(maps.get("desc_map")), _ptr(maps.get("peak0")), _ptr(maps.get("peak1")), _ptr(maps.get("peak2")), _ptr(maps.get("prob")), int(layer),
                _ptr(maps.get("layer_raw")), _ptr(maps.get("layer_norm")), _ptr(ws), ws.numel(),
            )  # fmt: skip
        out.update(maps)
        return out

    def _probe_ws(self, lib, B, H, W, dev):
        return self._ws.use(lib.imcui_hip_darkfeat_probe_workspace_bytes(B, H, W), dev)

    def stem_probe(self, packed: torch.Tensor, image: torch.Tensor) -> dict:
        """Test entry: image statistics and layer 0, image [B,3,H,W] -> raw [B,H,W,32] (before InstanceNorm), imstat [B,2], status [1]."""
        hd = get_handle(image.device)
        image = image.contiguous().float()
        B, _, H, W = image.shape
        f32 = dict(dtype=torch.float32, device=image.device)
        o = dict(raw=torch.empty((B, H, W, 32), **f32), imstat=torch.empty((B, 2), **f32), status=torch.zeros((1,), dtype=torch.int32, device=image.device))
        with self._probe_ws(hd.lib, B, H, W, image.device) as ws:
            hd.launch(hd.lib.imcui_hip_darkfeat_stem_probe, _ptr(packed), _ptr(image), B, H, W, _ptr(o["raw"]), _ptr(o["imstat"]), _ptr(o["status"]), _ptr(ws), ws.numel())
        return o

    def inorm_probe(self, x: torch.Tensor):
        """Test entry: InstanceNorm + ReLU of x [B,H,W,C] (NHWC, C = 32 / 64 / 128) -> (out [B,H,W,C], stat [B,C,2] = mean, rsqrt(var + eps))."""
        hd = get_handle(x.device)
        x = x.contiguous().float()
        B, H, W, Cc = x.shape
        out, stat = torch.empty_like(x), torch.empty((B, Cc, 2), dtype=torch.float32, device=x.device)
        with self._probe_ws(hd.lib, B, H, W, x.device) as ws:
            hd.launch(hd.lib.imcui_hip_darkfeat_inorm_probe, _ptr(x), B, H, W, Cc, _ptr(out), _ptr(stat), _ptr(ws), ws.numel())
        return out, stat

    def peak_probe(self, x: torch.Tensor, d: int, mavg: float) -> torch.Tensor:
        """Test entry: the peakiness pass on a raw map x [B,H,W,C] with dilation d and divisor mavg -> [B,H,W]."""
        hd = get_handle(x.device)
        x = x.contiguous().float()
        B, H, W, Cc = x.shape
        m = torch.tensor([mavg], dtype=torch.float32, device=x.device)
        out = torch.empty((B, H, W), dtype=torch.float32, device=x.device)
        hd.launch(hd.lib.imcui_hip_darkfeat_peak_probe, _ptr(x), _ptr(m), B, H, W, Cc, int(d), _ptr(out))
        return out

    def score_probe(self, packed: torch.Tensor, pk0: torch.Tensor, pk1: torch.Tensor, pk2: torch.Tensor, dmap: torch.Tensor) -> torch.Tensor:
        """Test entry: the score assembly from level maps pk0 [B,H,W], pk1 [B,h2,w2], pk2 [B,h4,w4] and dmap [B,h4,w4,128] -> [B,H,W]."""
        hd = get_handle(pk0.device)
        pk0, pk1, pk2, dmap = (t.contiguous().float() for t in (pk0, pk1, pk2, dmap))
        B, H, W = pk0.shape
        h2, w2, h4, w4 = darkfeat_map_sizes(H, W)
        if tuple(pk1.shape) != (B, h2, w2) or tuple(pk2.shape) != (B, h4, w4) or tuple(dmap.shape) != (B, h4, w4, DARKFEAT_DIM):
            raise ValueError("score_probe: the level maps do not have the sizes of the stride-2 chain")
        out = torch.empty((B, H, W), dtype=torch.float32, device=pk0.device)
        with self._probe_ws(hd.lib, B, H, W, pk0.device) as ws:
            hd.launch(hd.lib.imcui_hip_darkfeat_score_probe, _ptr(packed), _ptr(pk0), _ptr(pk1), _ptr(pk2), _ptr(dmap), B, H, W, _ptr(out), _ptr(ws), ws.numel())
        return out

    def detect_probe(self, score: torch.Tensor, conf: dict | None = None) -> dict:
        """Test entry: the detector, the cut and the ranked rows on a score map [B,H,W]; conf: max_keypoints and the detector keys."""
        conf = dict(conf or {})
        maxk = int(conf.get("max_keypoints") or 0)
        if maxk < 0:
            raise ValueError(f"DarkFeat: max_keypoints={maxk} is negative; 0 keeps every key-point")
        det = darkfeat_det_conf(conf)
        hd = get_handle(score.device)
        score = score.contiguous().float()
        B, H, W = score.shape
        dev = score.device
        kout = _darkfeat_kout(H * W, det, maxk)
        kpts, scores, _, nk, status, out = _sparse_outputs(B, kout, 1, dev)
        out.pop("descriptors")
        out["num_candidates"] = torch.empty((B,), dtype=torch.int32, device=dev)
        out["det_map"] = torch.empty((B, H, W), dtype=torch.float32, device=dev)
        with self._probe_ws(hd.lib, B, H, W, dev) as ws:
            hd.launch(hd.lib.imcui_hip_darkfeat_detect_probe, _ptr(score), B, H, W, float(det["score_thld"]), float(det["edge_thld"]), int(det["nms_size"]),
                      int(det["eof_mask"]), int(det["kpt_n"]), maxk, kout, _ptr(kpts), _ptr(scores), _ptr(nk), _ptr(out["num_candidates"]), _ptr(status),
                      _ptr(out["det_map"]), _ptr(ws), ws.numel())  # fmt: skip
        return out

    def describe_probe(self, dmap: torch.Tensor, keypoints: torch.Tensor, nkpts: torch.Tensor) -> torch.Tensor:
        """Test entry: descriptors at keypoints [B,K,2] (x, y in image pixels; nkpts [B] valid rows) of a map dmap [B,h4,w4,128]."""
        hd = get_handle(dmap.device)
        dmap, keypoints = dmap.contiguous().float(), keypoints.contiguous().float()
        nkpts = nkpts.to(dmap.device, torch.int32).contiguous()
        B, h4, w4, _ = dmap.shape
        K = keypoints.shape[1]
        out = torch.empty((B, K, DARKFEAT_DIM), dtype=torch.float32, device=dmap.device)
        hd.launch(hd.lib.imcui_hip_darkfeat_describe_probe, _ptr(dmap), B, h4, w4, _ptr(keypoints), _ptr(nkpts), K, _ptr(out))
        return out


# ------------------------------------------------------------------ SFD2
SFD2_DIM = 128
SFD2_MIN_SIDE = 16
SFD2_TRUNK = ("conv1a", "conv1b", "conv2a", "conv2b", "conv3a", "conv3b")
SFD2_SELECT_DEFAULTS = {"min_keypoints": 128, "remove_borders": 4}  # backend-only conf keys (upstream's text is not at hand)
SFD2_KINDS = ("stem", "conv3x3", "conv1x1", "grouped3x3", "heads")


def sfd2_config(sd: dict) -> dict:
    """What an SFD2 (ResNet4x) state dict decides, read from its shapes: trunk widths, bottleneck count, channels per group, hidden width
    of the heads, kernel size of convPb / convDb, BatchNorm and bias.  Nothing is guessed: a missing key or an unexpected shape raises."""

    def shape(name):
        if name not in sd:
            raise ImcuiHipError(f"SFD2 state dict: '{name}' is missing")
        s = tuple(sd[name].shape)
        if len(s) != 4 or s[2] != s[3]:
            raise ImcuiHipError(f"SFD2 state dict: '{name}' has shape {s}, expected a square convolution kernel [cout, cin, k, k]")
        return s

    c1, c2, c3 = (shape(f"conv{i}b.0.weight")[0] for i in (1, 2, 3))
    nb = 0
    while f"conv4.{nb}.conv1.weight" in sd:
        nb += 1
    cg = shape("conv4.0.conv2.weight")[1] if nb else 8  # (no bottleneck: no grouped layer is launched, the value is read by nobody)
    ch = shape("convPa.0.weight")[0]
    if shape("convDa.0.weight")[0] != ch:
        raise ImcuiHipError(f"SFD2: convPa is {ch} wide and convDa {shape('convDa.0.weight')[0]}: the two hidden layers run as one launch and need one width")
    pb, db = shape("convPb.weight"), shape("convDb.weight")
    if pb[0] != 16 or db[0] != SFD2_DIM:
        raise ImcuiHipError(f"SFD2: convPb has {pb[0]} outputs (16: a 4 x 4 depth-to-space) and convDb {db[0]} ({SFD2_DIM})")
    for name, s in (("convPb", pb), ("convDb", db)):
        if s[2] not in (1, 3):
            raise ImcuiHipError(f"SFD2: {name}.weight has shape {s}: the kernel must be 1x1 or 3x3")
    cfg = {"widths": (c1, c2, c3), "blocks": nb, "group_channels": cg, "hidden": ch, "k": (pb[2], db[2]), "bn": int("conv1a.1.weight" in sd),
           "bias": int("conv1a.0.bias" in sd), "block_bias": int("conv4.0.conv1.bias" in sd)}  # fmt: skip
    if load_library().imcui_hip_sfd2_packed_floats(sfd2_cfg_array(cfg)) == 0:
        raise ImcuiHipError(f"SFD2: the library refuses the configuration {cfg} (c1 = 64, widths multiples of 32 up to 512, up to 8 bottlenecks, "
                            "4 / 8 / 16 channels per group)")  # fmt: skip
    return cfg


def sfd2_cfg_array(cfg: dict):
    """The 12 ints of include/imcui_hip.h's `cfg`."""
    return (C.c_int * 12)(*cfg["widths"], cfg["blocks"], cfg["group_channels"], cfg["hidden"], *cfg["k"], cfg["bn"], cfg["bias"], cfg["block_bias"], 0)


def sfd2_layers(cfg: dict) -> list[dict]:
    """The launch list as the library's ONE table states it (csrc/sfd2.hip, SFD2_LAYERS): name, kind, cin, cout, stride, block (0 none,
    1 / 2 / 3 = first / middle / last launch of a bottleneck)."""
    lib, ca = load_library(), sfd2_cfg_array(cfg)
    out = []
    for i in range(lib.imcui_hip_sfd2_num_layers(ca)):
        v = (C.c_int * 5)()
        name = lib.imcui_hip_sfd2_layer(ca, i, v).decode()
        out.append({"name": name, "kind": SFD2_KINDS[v[0]], "cin": v[1], "cout": v[2], "stride": v[3], "block": v[4]})
    return out


def sfd2_tensor_names(cfg: dict) -> list[str]:
    lib, ca = load_library(), sfd2_cfg_array(cfg)
    return [lib.imcui_hip_sfd2_tensor_name(ca, i).decode() for i in range(lib.imcui_hip_sfd2_num_tensors(ca))]


def sfd2_tensor_shapes(cfg: dict) -> dict:
    shapes = {}

    def conv(stem, bn, cout, cin, k, bias):
        shapes[f"{stem}.weight"] = (cout, cin, k, k)
        if bias:
            shapes[f"{stem}.bias"] = (cout,)
        if cfg["bn"]:
            for key in _BN_KEYS:
                shapes[f"{bn}.{key}"] = (cout,)

    c3, ch, cg = cfg["widths"][2], cfg["hidden"], cfg["group_channels"]
    for L in sfd2_layers(cfg):
        if L["kind"] == "heads":
            conv("convPa.0", "convPa.1", ch, c3, 3, cfg["bias"])
            conv("convDa.0", "convDa.1", ch, c3, 3, cfg["bias"])
        elif L["block"]:
            stem = L["name"]  # conv4.{i}.conv{j}
            conv(stem, stem.replace(".conv", ".bn"), L["cout"], cg if L["kind"] == "grouped3x3" else L["cin"], 1 if L["kind"] == "conv1x1" else 3, cfg["block_bias"])
        else:
            stem = L["name"]  # conv1a.0
            conv(stem, stem[:-1] + "1", L["cout"], L["cin"], 3, cfg["bias"])
    shapes["convPb.weight"], shapes["convPb.bias"] = (16, ch, cfg["k"][0], cfg["k"][0]), (16,)
    shapes["convDb.weight"], shapes["convDb.bias"] = (SFD2_DIM, ch, cfg["k"][1], cfg["k"][1]), (SFD2_DIM,)
    return shapes


def pack_sfd2(state_dict: dict):
    """SFD2 state dict under upstream's keys (the plugin's SFD2_KEYS table admits them) -> (packed float32 buffer (host), cfg).  BatchNorm
    (eval) is folded by the packer.  Strict: `num_batches_tracked` counters are ignored, a convPb / convDb bias the checkpoint does not
    carry is zero, every other key is consumed exactly once and every shape checked; an unknown or missing key raises."""
    lib = load_library()
    sd = {k: t for k, t in state_dict.items() if not k.endswith("num_batches_tracked")}
    cfg = sfd2_config(sd)
    sd.setdefault("convPb.bias", torch.zeros(16))
    sd.setdefault("convDb.bias", torch.zeros(SFD2_DIM))
    ca = sfd2_cfg_array(cfg)
    return _pack_named("SFD2", "the ResNet4x", sfd2_tensor_names(cfg), sfd2_tensor_shapes(cfg), sd, lib.imcui_hip_sfd2_packed_floats(ca), lib.imcui_hip_sfd2_pack_weights, ca), cfg


def sfd2_pack_group(w: torch.Tensor) -> torch.Tensor:
    """Grouped 3x3 weights [C, CG, 3, 3] (OIHW per group) -> the packed order [group][tap][ci][co] of csrc/sfd2.hip."""
    Cc, cg = w.shape[:2]
    return w.reshape(Cc // cg, cg, cg, 9).permute(0, 3, 2, 1).contiguous()


def sfd2_map_sizes(H: int, W: int) -> tuple:
    """(h2, w2, Hc, Wc): a stride-2 layer leaves (n - 1) // 2 + 1 rows / columns; the score map is (4 Hc, 4 Wc)."""
    h2, w2 = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    return h2, w2, (h2 - 1) // 2 + 1, (w2 - 1) // 2 + 1


def sfd2_select_conf(conf: dict) -> dict:
    """conf_th, max_keypoints and the backend-only keys min_keypoints / remove_borders of a conf; refusals by name."""
    if conf.get("multiscale"):
        raise ValueError("SFD2: multiscale is not served by the HIP backend")
    d = {"conf_th": float(conf.get("conf_th", 0.001)), "max_keypoints": int(conf.get("max_keypoints") or 0),
         **{k: int(conf.get(k, v)) for k, v in SFD2_SELECT_DEFAULTS.items()}}  # fmt: skip
    if d["max_keypoints"] < 0:
        raise ValueError(f"SFD2: max_keypoints={d['max_keypoints']} is negative; 0 keeps every key-point")
    if d["min_keypoints"] < 0 or d["remove_borders"] < 0 or not d["conf_th"] >= 0:
        raise ValueError(f"SFD2: min_keypoints={d['min_keypoints']} (>= 0), remove_borders={d['remove_borders']} (>= 0), conf_th={d['conf_th']} (>= 0)")
    return d


def sfd2_check_args(image_shape) -> None:
    """Refusals raised before anything is launched."""
    if len(image_shape) != 4 or image_shape[1] != 3:
        raise ValueError(f"SFD2 expects an RGB image [B,3,H,W], got shape {tuple(image_shape)}")
    if image_shape[2] < SFD2_MIN_SIDE or image_shape[3] < SFD2_MIN_SIDE:
        raise ValueError(f"SFD2 needs images of at least {SFD2_MIN_SIDE} x {SFD2_MIN_SIDE}, got {tuple(image_shape[2:])}")


class Sfd2HIP:
    def __init__(self, cfg: dict):
        self.cfg = cfg
        self._ca = sfd2_cfg_array(cfg)
        self._ws = _Workspace()

    def forward(self, packed: torch.Tensor, image: torch.Tensor, conf: dict, want_maps: bool = False, layer: int = -1):
        """image [B,3,H,W] float32 RGB in [0,1] on the GPU -> fixed-stride outputs, no host synchronisation: keypoints [B,K,2] (x, y in
        pixels, integer-valued), scores [B,K], descriptors [B,K,128], num_keypoints [B] int32, status [1] int32 (always 0), rows in
        descending score order (equal scores by ascending pixel index), rows past the count zero.  K = min(max_keypoints or all, score-map
        pixels).  want_maps adds score [B,4Hc,4Wc] and desc_map [B,Hc,Wc,128] (normalised); `layer` adds layer_out, the NHWC output of
        that launch of `sfd2_layers`."""
        sel = sfd2_select_conf(conf)
        sfd2_check_args(tuple(image.shape))
        hd = get_handle(image.device)
        _same_device(packed, image)
        lib = hd.lib
        image = image.contiguous().float()
        B, Cc, H, W = image.shape
        dev = image.device
        _, _, Hc, Wc = sfd2_map_sizes(H, W)
        np_ = 16 * Hc * Wc
        kout = max(1, min(sel["max_keypoints"], np_) if sel["max_keypoints"] > 0 else np_)
        kpts, scores, desc, nk, status, out = _sparse_outputs(B, kout, SFD2_DIM, dev)
        f32 = dict(dtype=torch.float32, device=dev)
        maps = {}
        if want_maps:
            maps = dict(score=torch.empty((B, 4 * Hc, 4 * Wc), **f32), desc_map=torch.empty((B, Hc, Wc, SFD2_DIM), **f32))
        if layer >= 0:
            hh, ww, sizes = H, W, []
            for L in sfd2_layers(self.cfg):
                if L["stride"] == 2:
                    hh, ww = (hh - 1) // 2 + 1, (ww - 1) // 2 + 1
                sizes.append((B, hh, ww, L["cout"]))
            maps["layer_out"] = torch.empty(sizes[layer], **f32)
        with self._ws.use(lib.imcui_hip_sfd2_workspace_bytes(self._ca, B, H, W), dev) as ws:
            hd.launch(
                lib.imcui_hip_sfd2_forward, self._ca, _ptr(packed), _ptr(image), B, Cc, H, W, sel["conf_th"], sel["remove_borders"], sel["min_keypoints"],
                sel["max_keypoints"], kout, _ptr(kpts), _ptr(scores), _ptr(desc), _ptr(nk), _ptr(status), _ptr(maps.get("score")), _ptr(maps.get("desc_map")),
                int(layer), _ptr(maps.get("layer_out")), _ptr(ws), ws.numel(),
            )  # fmt: skip
        out.update(maps)
        return out

    def gconv_probe(self, x: torch.Tensor, w: torch.Tensor, shift: torch.Tensor, relu: bool) -> torch.Tensor:
        """Test entry: the grouped 3x3 convolution of x [B,H,W,C] (NHWC) with OIHW group weights w [C,CG,3,3] and shift [C]."""
        hd = get_handle(x.device)
        x, shift = x.contiguous().float(), shift.contiguous().float()
        wp = sfd2_pack_group(w.float()).to(x.device)
        B, H, W, Cc = x.shape
        out = torch.empty_like(x)
        hd.launch(hd.lib.imcui_hip_sfd2_gconv_probe, _ptr(x), _ptr(wp), _ptr(shift), B, H, W, Cc, int(w.shape[1]), int(bool(relu)), _ptr(out))
        return out

    def layers_probe(self, packed: torch.Tensor, x: torch.Tensor, first: int, last: int) -> torch.Tensor:
        """Test entry: launches [first, last] of the forward's own list on x: the planar image [B,3,H,W] when first == 0, else an NHWC map
        [B,H,W,cin] -> the last launch's NHWC map."""
        hd = get_handle(x.device)
        x = x.contiguous().float()
        B, H, W = (x.shape[0], x.shape[2], x.shape[3]) if first == 0 else tuple(x.shape[:3])
        hh, ww = H, W
        layers = sfd2_layers(self.cfg)
        for L in layers[first : last + 1]:
            if L["stride"] == 2:
                hh, ww = (hh - 1) // 2 + 1, (ww - 1) // 2 + 1
        out = torch.empty((B, hh, ww, layers[last]["cout"]), dtype=torch.float32, device=x.device)
        with self._ws.use(hd.lib.imcui_hip_sfd2_layers_workspace_bytes(self._ca, first, last, B, H, W), x.device) as ws:
            hd.launch(hd.lib.imcui_hip_sfd2_layers_probe, self._ca, _ptr(packed), _ptr(x), first, last, B, H, W, _ptr(out), _ptr(ws), ws.numel())
        return out

    @staticmethod
    def score_probe(logits: torch.Tensor) -> torch.Tensor:
        """Test entry: logits [B,Hc,Wc,16] -> score [B,4Hc,4Wc] (sigmoid, depth-to-space with channel 4 dy + dx)."""
        hd = get_handle(logits.device)
        logits = logits.contiguous().float()
        B, Hc, Wc, _ = logits.shape
        out = torch.empty((B, 4 * Hc, 4 * Wc), dtype=torch.float32, device=logits.device)
        hd.launch(hd.lib.imcui_hip_sfd2_score_probe, _ptr(logits), B, Hc, Wc, _ptr(out))
        return out

    def select_probe(self, score: torch.Tensor, image_size: tuple, conf: dict | None = None) -> dict:
        """Test entry: NMS, fallback, cut and ranked rows on a score map [B,Hs,Ws] of images of image_size = (H, W)."""
        sel = sfd2_select_conf(dict(conf or {}))
        hd = get_handle(score.device)
        score = score.contiguous().float()
        B, Hs, Ws = score.shape
        H, W = image_size
        dev = score.device
        kout = max(1, min(sel["max_keypoints"], Hs * Ws) if sel["max_keypoints"] > 0 else Hs * Ws)
        kpts, scores, _, nk, status, out = _sparse_outputs(B, kout, 1, dev)
        out.pop("descriptors")
        out["num_candidates"] = torch.empty((B,), dtype=torch.int32, device=dev)
        out["threshold"] = torch.empty((B,), dtype=torch.float32, device=dev)
        out["nms"] = torch.empty((B, Hs, Ws), dtype=torch.float32, device=dev)
        with self._ws.use(hd.lib.imcui_hip_sfd2_select_workspace_bytes(B, Hs, Ws), dev) as ws:
            hd.launch(hd.lib.imcui_hip_sfd2_select_probe, _ptr(score), B, Hs, Ws, int(H), int(W), sel["conf_th"], sel["remove_borders"], sel["min_keypoints"],
                      sel["max_keypoints"], kout, _ptr(kpts), _ptr(scores), _ptr(nk), _ptr(out["num_candidates"]), _ptr(out["threshold"]), _ptr(status),
                      _ptr(out["nms"]), _ptr(ws), ws.numel())  # fmt: skip
        return out

    @staticmethod
    def describe_probe(dmap: torch.Tensor, keypoints: torch.Tensor, nkpts: torch.Tensor, normalise: bool = True):
        """Test entry: descriptors at keypoints [B,K,2] (x, y in image pixels; nkpts [B] valid rows) of a map dmap [B,h4,w4,128]
        -> (descriptors [B,K,128], the map the sampler read: normalised over channels when `normalise`)."""
        hd = get_handle(dmap.device)
        dmap, keypoints = dmap.contiguous().float(), keypoints.contiguous().float()
        nkpts = nkpts.to(dmap.device, torch.int32).contiguous()
        B, h4, w4, _ = dmap.shape
        K = keypoints.shape[1]
        out = torch.empty((B, K, SFD2_DIM), dtype=torch.float32, device=dmap.device)
        dn = torch.empty_like(dmap) if normalise else None
        hd.launch(hd.lib.imcui_hip_sfd2_describe_probe, _ptr(dmap), B, h4, w4, int(bool(normalise)), _ptr(dn), _ptr(keypoints), _ptr(nkpts), K, _ptr(out))
        return out, (dn if normalise else dmap)


# ------------------------------------------------------------------ NetVLAD
# (cin, cout, index in torchvision's vgg16().features): VGG-16 to conv5_3, csrc/netvlad.hip
NETVLAD_LAYERS = ((3, 64, 0), (64, 64, 2), (64, 128, 5), (128, 128, 7), (128, 256, 10), (256, 256, 12), (256, 256, 14), (256, 512, 17), (512, 512, 19),
                  (512, 512, 21), (512, 512, 24), (512, 512, 26), (512, 512, 28))  # fmt: skip
NETVLAD_DIM, NETVLAD_CLUSTERS, NETVLAD_WHITENED = 512, 64, 4096
NETVLAD_MIN_SIDE = 16  # four flooring 2x2 pools: a smaller side leaves an empty conv5_3 map


def netvlad_tensor_names(whiten: bool = True) -> list[str]:
    lib = load_library()
    return [lib.imcui_hip_netvlad_tensor_name(int(whiten), i).decode() for i in range(lib.imcui_hip_netvlad_num_tensors(int(whiten)))]


def netvlad_tensor_shapes(whiten: bool = True) -> dict:
    """The state-dict shapes of the reference's `NetVLAD` module (imcui/hloc/extractors/netvlad.py:64-114) + `preprocess.mean` (:118)."""
    shapes = {}
    for cin, cout, op in NETVLAD_LAYERS:
        shapes[f"backbone.{op}.weight"] = (cout, cin, 3, 3)
        shapes[f"backbone.{op}.bias"] = (cout,)
    shapes["netvlad.score_proj.weight"] = (NETVLAD_CLUSTERS, NETVLAD_DIM, 1)
    shapes["netvlad.centers"] = (NETVLAD_DIM, NETVLAD_CLUSTERS)
    shapes["preprocess.mean"] = (3,)
    if whiten:
        shapes["whiten.weight"] = (NETVLAD_WHITENED, NETVLAD_DIM * NETVLAD_CLUSTERS)
        shapes["whiten.bias"] = (NETVLAD_WHITENED,)
    return shapes


def pack_netvlad(state_dict: dict, whiten: bool | None = None) -> torch.Tensor:
    """The reference module's state dict (+ `preprocess.mean`) -> packed float32 buffer (host).  whiten None: by the presence of
    `whiten.weight`.  Strict: every key is consumed exactly once, every shape checked.  The whitening matrix (512 MB) is packed as float32."""
    lib = load_library()
    sd = dict(state_dict)
    if whiten is None:
        whiten = "whiten.weight" in sd
    w = int(bool(whiten))
    return _pack_named("NetVLAD", "the reference's NetVLAD module", netvlad_tensor_names(bool(w)), netvlad_tensor_shapes(bool(w)), sd,
                       lib.imcui_hip_netvlad_packed_floats(w), lib.imcui_hip_netvlad_pack_weights, w)


def netvlad_check_args(image_shape) -> None:
    """Refusals raised before anything is launched (the library refuses the same)."""
    if len(image_shape) != 4 or image_shape[1] != 3:
        raise ValueError(f"NetVLAD expects an RGB image [B,3,H,W], got shape {tuple(image_shape)}")
    if min(image_shape[2], image_shape[3]) < NETVLAD_MIN_SIDE:
        raise ValueError(f"NetVLAD: a {image_shape[2]}x{image_shape[3]} image has an empty conv5_3 map: every side needs at least {NETVLAD_MIN_SIDE} pixels")


class NetVLADHIP:
    def __init__(self):
        self._ws = _Workspace()

    def forward_batched(self, packed: torch.Tensor, image: torch.Tensor, whiten: bool, want_map: bool = False) -> dict:
        """image [B,3,H,W] float32 RGB in [0,1] on the GPU -> {"global_descriptor": [B,4096] (whiten) or [B,32768]}, unit norm; no host
        synchronisation, graph-capturable.  want_map adds `backbone` [B,H//16,W//16,512], the conv5_3 map (NHWC)."""
        netvlad_check_args(tuple(image.shape))
        hd = get_handle(image.device)
        _same_device(packed, image)
        lib = hd.lib
        w = int(bool(whiten))
        if packed.numel() != lib.imcui_hip_netvlad_packed_floats(w):
            raise ImcuiHipError(f"NetVLAD: the packed buffer holds {packed.numel()} floats, whiten={bool(w)} needs {lib.imcui_hip_netvlad_packed_floats(w)}")
        image = image.contiguous().float()
        B, Cc, H, W = image.shape
        dev = image.device
        desc = torch.empty((B, NETVLAD_WHITENED if w else NETVLAD_DIM * NETVLAD_CLUSTERS), dtype=torch.float32, device=dev)
        fmap = torch.empty((B, H // 16, W // 16, NETVLAD_DIM), dtype=torch.float32, device=dev) if want_map else None
        with self._ws.use(lib.imcui_hip_netvlad_workspace_bytes(B, H, W, w), dev) as ws:
            hd.launch(lib.imcui_hip_netvlad_forward, _ptr(packed), _ptr(image), B, Cc, H, W, w, _ptr(desc), _ptr(fmap), _ptr(ws), ws.numel())
        out = {"global_descriptor": desc}
        if want_map:
            out["backbone"] = fmap
        return out

    def layer_probe(self, op: str, inp: torch.Tensor, packed: torch.Tensor | None = None) -> torch.Tensor:
        """Test entry: one stage alone.  "conv0": image [B,3,H,W] -> [B,H,W,64]; "maxpool": NHWC [B,H,W,C] -> [B,H//2,W//2,C]; "vlad": maps
        [B,h,w,512] -> [B,32768] (pre-normalisation, assignment, aggregation, both normalisations); "conv5_3": maps [B,h,w,512] ->
        [B,h,w,512], the last convolution (no ReLU) as the forward launches it (K summed in groups), in the handle's arithmetic mode.
        All but maxpool need `packed`."""
        code = {"conv0": 0, "maxpool": 1, "vlad": 2, "conv5_3": 3}[op]
        hd = get_handle(inp.device)
        lib = hd.lib
        inp = inp.contiguous().float()
        if code == 0:
            B, _, H, W = inp.shape
            Cc, shape = 64, (B, H, W, 64)
        else:
            B, H, W, Cc = inp.shape
            shape = (B, H // 2, W // 2, Cc) if code == 1 else (B, NETVLAD_DIM * NETVLAD_CLUSTERS) if code == 2 else (B, H, W, Cc)
        out = torch.empty(shape, dtype=torch.float32, device=inp.device)
        with self._ws.use(max(256, lib.imcui_hip_netvlad_probe_workspace_bytes(B, H * W) if code >= 2 else 256), inp.device) as ws:
            hd.launch(lib.imcui_hip_netvlad_layer_probe, code, _ptr(packed), _ptr(inp), B, H, W, Cc, _ptr(out), _ptr(ws), ws.numel())
        return out

    def whiten_probe(self, weight: torch.Tensor, bias: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
        """Test entry: normalize(weight [out,in] @ x [B,in] + bias) through the split-K skinny GEMM and its fold -> [B,out]."""
        hd = get_handle(x.device)
        lib = hd.lib
        weight, bias, x = weight.contiguous().float(), bias.contiguous().float(), x.contiguous().float()
        (out_dim, in_dim), B = weight.shape, x.shape[0]
        if x.shape[1] != in_dim or bias.shape != (out_dim,):
            raise ValueError(f"whiten_probe: weight {tuple(weight.shape)}, bias {tuple(bias.shape)}, x {tuple(x.shape)}")
        out = torch.empty((B, out_dim), dtype=torch.float32, device=x.device)
        with self._ws.use(lib.imcui_hip_netvlad_whiten_workspace_bytes(B, in_dim, out_dim), x.device) as ws:
            hd.launch(lib.imcui_hip_netvlad_whiten_probe, _ptr(weight), _ptr(bias), _ptr(x), B, in_dim, out_dim, _ptr(out), _ptr(ws), ws.numel())
        return out


# ------------------------------------------------------------------ CosPlace / EigenPlaces
PLACES_BACKBONES = {"ResNet18": 18, "ResNet50": 50, "ResNet101": 101, "ResNet152": 152}  # conf["backbone"] -> the library's code
PLACES_DEPTHS = {18: (2, 2, 2, 2), 50: (3, 4, 6, 3), 101: (3, 4, 23, 3), 152: (3, 8, 36, 3)}  # torchvision's resnetNN `layers`


def places_backbone_code(backbone) -> int:
    """"ResNet50" (or 50) -> 50.  The VGG16 checkpoints of upstream are refused by name: that trunk is not built."""
    if isinstance(backbone, str) and backbone.lower() == "vgg16":
        raise ValueError("CosPlace / EigenPlaces: the VGG16 backbone is not built; use ResNet18, ResNet50, ResNet101 or ResNet152")
    code = PLACES_BACKBONES.get(backbone, backbone)
    if code not in PLACES_DEPTHS:
        raise ValueError(f"CosPlace / EigenPlaces: unknown backbone {backbone!r}; use ResNet18, ResNet50, ResNet101 or ResNet152")
    return code


def places_feature_dim(backbone) -> int:
    return 512 if places_backbone_code(backbone) == 18 else 2048


def places_map_size(h: int, w: int) -> tuple:
    """Sizes after conv1, the max-pool, layer2, layer3 and layer4: each (n - 1) // 2 + 1 of the one before."""
    out = []
    for _ in range(5):
        h, w = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        out.append((h, w))
    return tuple(out)


def places_tensor_names(backbone, fc_output_dim: int) -> list[str]:
    lib, code = load_library(), places_backbone_code(backbone)
    return [lib.imcui_hip_places_tensor_name(code, fc_output_dim, i).decode() for i in range(lib.imcui_hip_places_num_tensors(code, fc_output_dim))]


def places_tensor_shapes(backbone, fc_output_dim: int) -> dict:
    """The state-dict shapes of upstream's GeoLocalizationNet on a torchvision ResNet (cosplace_model/network.py), restated."""
    code = places_backbone_code(backbone)
    bott = code != 18
    shapes = {"backbone.0.weight": (64, 3, 7, 7)}

    def bn(prefix, c):
        for k in ("weight", "bias", "running_mean", "running_var"):
            shapes[f"{prefix}.{k}"] = (c,)

    bn("backbone.1", 64)
    cin = 64
    for L, depth in enumerate(PLACES_DEPTHS[code]):
        width = 64 << L
        cout = 4 * width if bott else width
        for i in range(depth):
            p, stride = f"backbone.{4 + L}.{i}", 2 if (i == 0 and L > 0) else 1
            convs = ((cin, width, 1), (width, width, 3), (width, cout, 1)) if bott else ((cin, width, 3), (width, width, 3))
            for j, (ci, co, k) in enumerate(convs, 1):
                shapes[f"{p}.conv{j}.weight"] = (co, ci, k, k)
                bn(f"{p}.bn{j}", co)
            if stride != 1 or cin != cout:
                shapes[f"{p}.downsample.0.weight"] = (cout, cin, 1, 1)
                bn(f"{p}.downsample.1", cout)
            cin = cout
    shapes["aggregation.1.p"] = (1,)
    shapes["aggregation.3.weight"] = (fc_output_dim, cin)
    shapes["aggregation.3.bias"] = (fc_output_dim,)
    return shapes


def pack_places(state_dict: dict, backbone, fc_output_dim: int) -> torch.Tensor:
    """Upstream's state dict (or a `{"state_dict": ...}` / `{"model_state_dict": ...}` wrapper of it) -> packed float32 buffer (host).
    `num_batches_tracked` entries are ignored.  Strict: every other key is consumed exactly once, every shape checked."""
    lib, code = load_library(), places_backbone_code(backbone)
    sd = state_dict
    for wrapper in ("state_dict", "model_state_dict"):
        if wrapper in sd and isinstance(sd[wrapper], dict):
            sd = sd[wrapper]
    sd = {k: v for k, v in sd.items() if not k.endswith("num_batches_tracked")}
    return _pack_named("CosPlace / EigenPlaces", f"the ResNet-{code} / {fc_output_dim}", places_tensor_names(code, fc_output_dim),
                       places_tensor_shapes(code, fc_output_dim), sd, lib.imcui_hip_places_packed_floats(code, fc_output_dim),
                       lib.imcui_hip_places_pack_weights, code, fc_output_dim)


def places_check_args(image_shape) -> None:
    """The refusal raised before anything is launched (the library refuses the same)."""
    if len(image_shape) != 4 or image_shape[1] != 3 or min(image_shape[2], image_shape[3]) < 1:
        raise ValueError(f"CosPlace / EigenPlaces expect an RGB image [B,3,H,W], got shape {tuple(image_shape)}")


class PlacesHIP:
    def __init__(self, backbone, fc_output_dim: int):
        self.code, self.dim = places_backbone_code(backbone), int(fc_output_dim)
        self.feat = places_feature_dim(self.code)
        self._ws = _Workspace()

    def _check_packed(self, lib, packed):
        need = lib.imcui_hip_places_packed_floats(self.code, self.dim)
        if packed.numel() != need:
            raise ImcuiHipError(f"CosPlace / EigenPlaces: the packed buffer holds {packed.numel()} floats, ResNet-{self.code} / {self.dim} needs {need}")

    def forward_batched(self, packed: torch.Tensor, image: torch.Tensor, want_map: bool = False) -> dict:
        """image [B,3,H,W] float32 RGB in [0,1] on the GPU -> {"global_descriptor": [B,fc_output_dim]}, unit norm; no host synchronisation,
        graph-capturable.  want_map adds `backbone` [B,h4,w4,F], the layer4 map (NHWC)."""
        places_check_args(tuple(image.shape))
        hd = get_handle(image.device)
        _same_device(packed, image)
        lib = hd.lib
        self._check_packed(lib, packed)
        image = image.contiguous().float()
        B, Cc, H, W = image.shape
        dev = image.device
        desc = torch.empty((B, self.dim), dtype=torch.float32, device=dev)
        fmap = torch.empty((B, *places_map_size(H, W)[-1], self.feat), dtype=torch.float32, device=dev) if want_map else None
        with self._ws.use(lib.imcui_hip_places_workspace_bytes(self.code, self.dim, B, H, W), dev) as ws:
            hd.launch(lib.imcui_hip_places_forward, _ptr(packed), _ptr(image), B, Cc, H, W, self.code, self.dim, _ptr(desc), _ptr(fmap), _ptr(ws), ws.numel())
        out = {"global_descriptor": desc}
        if want_map:
            out["backbone"] = fmap
        return out

    def layer_probe(self, op: str, inp: torch.Tensor, packed: torch.Tensor, layer: int = 0, block: int = 0) -> torch.Tensor:
        """Test entry: one stage alone.  "stem": image [B,3,H,W] -> [B,Hp,Wp,64]; "block": NHWC [B,H,W,cin] -> [B,Ho,Wo,cout], block `block`
        of layer 1 .. 4 in the handle's arithmetic mode; "gem": [B,H,W,F] -> [B,F]; "head": [B,F] -> [B,fc_output_dim]."""
        code = {"stem": 0, "block": 1, "gem": 2, "head": 3}[op]
        hd = get_handle(inp.device)
        lib = hd.lib
        self._check_packed(lib, packed)
        inp = inp.contiguous().float()
        key = f"backbone.{3 + layer}.{block}.conv1.weight"
        shapes = places_tensor_shapes(self.code, self.dim) if code == 1 else {}
        want_c = 3 if code == 0 else shapes.get(key, (0, -1))[1] if code == 1 else self.feat
        if inp.dim() != (2 if code == 3 else 4) or inp.shape[1 if code in (0, 3) else 3] != want_c:
            raise ValueError(f"places layer probe '{op}' (layer {layer}, block {block}): input {tuple(inp.shape)}, {want_c} channels expected")
        if code == 0:
            B, _, H, W = inp.shape
            shape = (B, *places_map_size(H, W)[1], 64)
        elif code == 1:
            B, H, W, _ = inp.shape
            bott, width = self.code != 18, 64 << (layer - 1)
            stride = 2 if (block == 0 and layer > 1) else 1
            shape = (B, (H - 1) // stride + 1, (W - 1) // stride + 1, 4 * width if bott else width)
        elif code == 2:
            B, H, W, _ = inp.shape
            shape = (B, self.feat)
        else:
            (B, _), H, W = inp.shape, 1, 1
            shape = (B, self.dim)
        out = torch.empty(shape, dtype=torch.float32, device=inp.device)
        with self._ws.use(max(256, lib.imcui_hip_places_probe_workspace_bytes(self.code, self.dim, code, B, H, W, layer, block)), inp.device) as ws:
            hd.launch(lib.imcui_hip_places_layer_probe, code, self.code, self.dim, _ptr(packed), _ptr(inp), B, H, W, layer, block, _ptr(out), _ptr(ws), ws.numel())
        return out


_retrieval_ws = _Workspace()


def retrieval_topk(query: torch.Tensor, db: torch.Tensor, num_select: int, invalid: torch.Tensor | None = None, min_score: float | None = None):
    """pairs_from_retrieval.py:109 + :56-66 on the device: query [Q,D], db [N,D] -> (indices [Q,num_select] int32, scores [Q,num_select]):
    the `num_select` highest similarities of every row in descending order, an `invalid` entry (bool / uint8 [Q,N]) or one below
    `min_score` counting as -inf; equal scores by ascending database index; slots past N hold -1 / -inf.  The score matrix is not returned."""
    hd = get_handle(query.device)
    lib = hd.lib
    _same_device(db, query)
    query, db = query.contiguous().float(), db.contiguous().float()
    (Q, D), N = query.shape, db.shape[0]
    if db.dim() != 2 or db.shape[1] != D or num_select < 1:
        raise ValueError(f"retrieval_topk: query {tuple(query.shape)}, db {tuple(db.shape)}, num_select {num_select}")
    inv = None
    if invalid is not None:
        if tuple(invalid.shape) != (Q, N):
            raise ValueError(f"retrieval_topk: invalid has shape {tuple(invalid.shape)}, expected {(Q, N)}")
        inv = invalid.to(query.device).to(torch.uint8).contiguous()
    idx = torch.empty((Q, num_select), dtype=torch.int32, device=query.device)
    sc = torch.empty((Q, num_select), dtype=torch.float32, device=query.device)
    with _retrieval_ws.use(lib.imcui_hip_retrieval_topk_workspace_bytes(Q, N), query.device) as ws:
        hd.launch(lib.imcui_hip_retrieval_topk, _ptr(query), _ptr(db), Q, N, D, _ptr(inv), int(min_score is not None),
                  float(min_score or 0.0), int(num_select), _ptr(idx), _ptr(sc), _ptr(ws), ws.numel())  # fmt: skip
    return idx, sc


# ------------------------------------------------------------------ DeDoDe
DEDODE_SCALES = (8, 4, 2, 1)
DEDODE_FEATURE_CHANNELS = (512, 256, 128, 64)  # the encoders' maps in front of the pools, at DEDODE_SCALES
DEDODE_MODELS = ("detector", "descriptor")
DEDODE_MODEL_NAMES = {"detector": "dedode_detector_L.pth", "descriptor": "dedode_descriptor_B.pth"}  # the sizes csrc/dedode.hip serves
# torchvision cfg "E" / "A" up to the fourth pool (vgg19_bn().features[:40], vgg11_bn().features[:22]); "M" = MaxPool2d(2, 2)
DEDODE_ENCODERS = {"detector": (64, 64, "M", 128, 128, "M", 256, 256, 256, 256, "M", 512, 512, 512, 512, "M"),
                   "descriptor": (64, "M", 128, "M", 256, 256, "M", 512, 512, "M")}  # fmt: skip
DEDODE_DESC_DIM = 256


def dedode_encoder_convs(model: str) -> list:
    """(index in vgg.features, cin, cout) of every convolution; its BatchNorm is at index + 1."""
    out, op, cin = [], 0, 3
    for v in DEDODE_ENCODERS[model]:
        if v == "M":
            op += 1
        else:
            out.append((op, cin, v))
            cin, op = v, op + 3
    return out


def dedode_dims(sd_detector: dict, sd_descriptor: dict) -> tuple:
    """The ConvRefiner shapes of both state dicts, READ from the tensors: per model and scale (8, 4, 2, 1) `in` and `hidden` from
    block1.0.weight, `out` from out_conv.weight and the number of hidden blocks from the keys -> the flat table the library takes."""
    dims = []
    for model, sd in zip(DEDODE_MODELS, (sd_detector, sd_descriptor)):
        for s in DEDODE_SCALES:
            p = f"decoder.layers.{s}."
            for key in (p + "block1.0.weight", p + "out_conv.weight"):
                if key not in sd or sd[key].dim() != 4:
                    raise ImcuiHipError(f"DeDoDe {model} state dict: missing '{key}' (a [rows,cols,1,1] convolution): the refiner of scale {s} cannot be read")
            hidden, cin = int(sd[p + "block1.0.weight"].shape[0]), int(sd[p + "block1.0.weight"].shape[1])
            n = 0
            while f"{p}hidden_blocks.{n}.0.weight" in sd:
                n += 1
            dims += [cin, hidden, int(sd[p + "out_conv.weight"].shape[0]), n]
    dims = tuple(dims)
    why = load_library().imcui_hip_dedode_dims_error(_dedode_cdims(dims)).decode()
    if why:
        raise ImcuiHipError(f"DeDoDe state dicts are not served: {why}")
    return dims


def _dedode_cdims(dims):
    return (C.c_int * 32)(*dims)


def dedode_tensor_names(dims) -> list[str]:
    lib, cd = load_library(), _dedode_cdims(dims)
    return [lib.imcui_hip_dedode_tensor_name(cd, i).decode() for i in range(lib.imcui_hip_dedode_num_tensors(cd))]


def dedode_tensor_shapes(dims) -> dict:
    shapes = {"density_taps": (51,)}

    def bn(p, c):
        for k in ("weight", "bias", "running_mean", "running_var"):
            shapes[f"{p}.{k}"] = (c,)

    def block(p, cin, c, depthwise):
        shapes[p + ".0.weight"] = (c, 1, 5, 5) if depthwise else (c, cin, 1, 1)
        shapes[p + ".0.bias"] = (c,)
        bn(p + ".1", c)
        shapes[p + ".3.weight"] = (c, c, 1, 1)
        shapes[p + ".3.bias"] = (c,)

    for m, model in enumerate(DEDODE_MODELS):
        for op, cin, cout in dedode_encoder_convs(model):
            shapes[f"{model}.encoder.layers.{op}.weight"] = (cout, cin, 3, 3)
            shapes[f"{model}.encoder.layers.{op}.bias"] = (cout,)
            bn(f"{model}.encoder.layers.{op + 1}", cout)
        for i, s in enumerate(DEDODE_SCALES):
            cin, hidden, out, n = dims[(m * 4 + i) * 4 : (m * 4 + i) * 4 + 4]
            p = f"{model}.decoder.layers.{s}"
            block(p + ".block1", cin, hidden, False)
            for j in range(n):
                block(f"{p}.hidden_blocks.{j}", hidden, hidden, True)
            shapes[p + ".out_conv.weight"] = (out, hidden, 1, 1)
            shapes[p + ".out_conv.bias"] = (out,)
    return shapes


def dedode_density_taps() -> torch.Tensor:
    """sample_keypoints' `(-torch.linspace(-2, 2, steps=51) ** 2).exp()`, float32 on the host: the library filters with these bits."""
    return torch.exp(-torch.linspace(-2, 2, 51, dtype=torch.float32) ** 2)


def pack_dedode(sd_detector: dict, sd_descriptor: dict):
    """The two DeDoDe state dicts -> (packed float32 buffer (host), dims).  Strict: every key is consumed exactly once and every shape is
    checked against the widths read from the refiners; only the BatchNorm `num_batches_tracked` counters are skipped."""
    lib = load_library()
    dims = dedode_dims(sd_detector, sd_descriptor)
    merged = {}
    for model, sd in zip(DEDODE_MODELS, (sd_detector, sd_descriptor)):
        merged.update({f"{model}.{k}": v for k, v in sd.items() if not k.endswith("num_batches_tracked")})
    merged["density_taps"] = dedode_density_taps()
    cd = _dedode_cdims(dims)
    packed = _pack_named("DeDoDe", "the detector L / descriptor B", dedode_tensor_names(dims), dedode_tensor_shapes(dims), merged,
                         lib.imcui_hip_dedode_packed_floats(cd), lib.imcui_hip_dedode_pack_weights, cd)  # fmt: skip
    return packed, dims


def dedode_check_args(image_shape, conf: dict) -> int:
    """Refusals raised before anything is launched; returns num_keypoints."""
    if conf.get("dense"):
        raise ValueError("DeDoDe: `dense: True` (detect_dense) is not served by the HIP backend; the reference fixes it to False")
    for key, model in (("model_detector_name", "detector"), ("model_descriptor_name", "descriptor")):
        if conf.get(key, DEDODE_MODEL_NAMES[model]) != DEDODE_MODEL_NAMES[model]:
            raise ValueError(f"DeDoDe: {key}={conf[key]!r} is not served, only {DEDODE_MODEL_NAMES[model]!r} (detector L with descriptor B)")
    if len(image_shape) != 4 or image_shape[1] != 3:
        raise ValueError(f"DeDoDe expects an RGB image [B,3,H,W], got shape {tuple(image_shape)}")
    H, W = int(image_shape[2]), int(image_shape[3])
    if H < 8 or W < 8 or H % 8 or W % 8:
        raise ValueError(f"DeDoDe: image sides {H}x{W} must be multiples of 8 (every `dedode` conf of the reference resizes with dfactor 8)")
    k = int(conf["max_keypoints"])
    if not 1 <= k <= H * W:
        raise ValueError(f"DeDoDe: max_keypoints={k} is out of range for a {H}x{W} image: topk over {H * W} pixels would raise")
    return k


class DeDoDeHIP:
    def __init__(self):
        self._ws = _Workspace()

    def forward(self, packed: torch.Tensor, dims, image: torch.Tensor, conf: dict, want_maps: bool = False, want_dense: bool = False, kout: int | None = None):
        """image [B,3,H,W] float32 RGB in [0,1] on the GPU -> fixed-stride outputs, no host synchronisation: keypoints [B,K,2] (x, y in
        pixels), scores [B,K], descriptors [B,K,256] (not normalised), num_keypoints [B] int32 (= max_keypoints: every pixel is a
        candidate), status [1] int32 (0), rows in descending score, ties by ascending pixel index; K = kout or max_keypoints, rows past
        the count zero.  want_maps adds `logits` (the detector's accumulated logits at scales 8, 4, 2, 1, each [B,h,w]), `logp`,
        `score` [B,H,W] and `desc2` [B,H/2,W/2,256]; want_dense adds `dense` [B,H,W,256], the grid the call otherwise never forms."""
        k = dedode_check_args(tuple(image.shape), conf)
        hd = get_handle(image.device)
        _same_device(packed, image)
        lib = hd.lib
        image = image.contiguous().float()
        B, _, H, W = image.shape
        dev = image.device
        kout = k if kout is None else int(kout)
        if kout < k:
            raise ValueError(f"DeDoDe: kout={kout} below max_keypoints={k}")
        kpts, scores, desc, nk, status, out = _sparse_outputs(B, kout, DEDODE_DESC_DIM, dev)
        cd = _dedode_cdims(dims)
        sizes = [(H // s, W // s) for s in DEDODE_SCALES]
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)  # noqa: E731
        logits = new(B * sum(a * b for a, b in sizes)) if want_maps else None
        logp, score, desc2 = (new(B, H, W), new(B, H, W), new(B, H // 2, W // 2, DEDODE_DESC_DIM)) if want_maps else (None, None, None)
        dense = new(B, H, W, DEDODE_DESC_DIM) if want_dense else None
        with self._ws.use(lib.imcui_hip_dedode_workspace_bytes(cd, B, H, W, k), dev) as ws:
            hd.launch(
                lib.imcui_hip_dedode_forward, _ptr(packed), cd, _ptr(image), B, H, W, k, kout, _ptr(kpts), _ptr(scores), _ptr(desc), _ptr(nk), _ptr(status),
                _ptr(logits), _ptr(logp), _ptr(score), _ptr(desc2), _ptr(dense), _ptr(ws), ws.numel(),
            )  # fmt: skip
        if want_maps:
            out["logits"], off = [], 0
            for a, b in sizes:
                out["logits"].append(logits[off : off + B * a * b].view(B, a, b))
                off += B * a * b
            out.update(logp=logp, score=score, desc2=desc2)
        if want_dense:
            out["dense"] = dense
        return out

    @staticmethod
    def layer_probe(op: str, inp: torch.Tensor, weights: torch.Tensor | None = None, packed: torch.Tensor | None = None, dims=None, model: str = "detector"):
        """Test entry: one of the new kernels alone.  "conv0": image [B,3,H,W] -> [B,H,W,64] (needs `packed`, `dims`, `model`);
        "depthwise": NHWC [B,H,W,C] with weights = cat([25,C] taps, [C] bias) -> ReLU(conv + bias); "bilinear2": NHWC -> [B,2H,2W,C];
        "bicubic2": [B,H,W] -> [B,2H,2W]; "softmax_stats": [B,H,W] -> [B,2] = (max, log sum exp(l - max)); "filter51": [B,H,W] with
        weights = the 51 taps -> [B,H,W]."""
        code = {"conv0": 0, "depthwise": 1, "bilinear2": 2, "bicubic2": 3, "softmax_stats": 4, "filter51": 5}[op]
        hd = get_handle(inp.device)
        inp = inp.contiguous().float()
        dev = inp.device
        if code == 0:
            B, _, H, W = inp.shape
            Cc, shape = 64, (B, H, W, 64)
        elif code in (1, 2):
            B, H, W, Cc = inp.shape
            shape = (B, H, W, Cc) if code == 1 else (B, 2 * H, 2 * W, Cc)
        else:
            B, H, W = inp.shape
            Cc = 1
            shape = {3: (B, 2 * H, 2 * W), 4: (2 * B + 2 * B * ((H * W + 4095) // 4096),), 5: (2, B, H, W)}[code]
        out = torch.empty(shape, dtype=torch.float32, device=dev)
        if weights is not None:
            weights = weights.contiguous().float().to(dev)
        cd = _dedode_cdims(dims) if dims is not None else None
        hd.launch(hd.lib.imcui_hip_dedode_layer_probe, code, _ptr(packed), cd, DEDODE_MODELS.index(model), _ptr(weights), _ptr(inp), B, H, W, Cc, _ptr(out))
        if code == 4:
            return out[: 2 * B].view(B, 2)
        return out[0] if code == 5 else out

    def select_probe(self, map_: torch.Tensor, k: int, mode: str = "logp", kout: int | None = None):
        """Test entry: the selection code on the caller's maps [B,H,W].  mode "logp": p = exp(log p), filter, score, cut, rows; mode
        "score": cut and rows on the given score map -> keypoints, scores, num_keypoints and the score map used."""
        hd = get_handle(map_.device)
        lib = hd.lib
        map_ = map_.contiguous().float()
        B, H, W = map_.shape
        dev = map_.device
        kout = k if kout is None else int(kout)
        kpts = torch.empty((B, kout, 2), dtype=torch.float32, device=dev)
        scores = torch.empty((B, kout), dtype=torch.float32, device=dev)
        nk = torch.empty((B,), dtype=torch.int32, device=dev)
        smap = torch.empty((B, H, W), dtype=torch.float32, device=dev)
        taps = dedode_density_taps().to(dev)
        with self._ws.use(lib.imcui_hip_dedode_select_probe_workspace_bytes(B, H, W, k), dev) as ws:
            hd.launch(lib.imcui_hip_dedode_select_probe, {"logp": 0, "score": 1}[mode], _ptr(taps), _ptr(map_), B, H, W, k, kout, _ptr(kpts), _ptr(scores),
                      _ptr(nk), _ptr(smap), _ptr(ws), ws.numel())  # fmt: skip
        return {"keypoints": kpts, "scores": scores, "num_keypoints": nk, "score": smap}


# ------------------------------------------------------------------ DoG + HardNet / SOSNet patch descriptors
PATCHDESC_MODELS = {"hardnet": 0, "sosnet": 1}
# (cin, cout, kernel) of the seven convolutions and their index in kornia's nn.Sequential (the BatchNorm2d(affine=False) follows at + 1):
# kornia.feature.HardNet.features / kornia.feature.SOSNet.layers (whose entry 0 is the InstanceNorm2d); csrc/dog.hip
PATCHDESC_LAYERS = ((1, 32, 3), (32, 32, 3), (32, 64, 3), (64, 64, 3), (64, 128, 3), (128, 128, 3), (128, 128, 8))
PATCHDESC_CONV_OPS = {"hardnet": (0, 3, 6, 9, 12, 15, 19), "sosnet": (1, 4, 7, 10, 13, 16, 20)}
PATCHDESC_ROOT = {"hardnet": "features", "sosnet": "layers"}
PATCHDESC_PROBE_OPS = {"pyrdown": 0, "norm": 1, "layer1": 2, "layer2": 3, "layer3": 4, "layer4": 5, "layer5": 6, "layer6": 7, "final": 8, "outnorm": 9}
PATCHDESC_CHUNK = 1024  # dog.py:35 `max_batch_size`
PATCHDESC_MAX_CHUNK = 8192


def patchdesc_model(name: str) -> int:
    if name not in PATCHDESC_MODELS:
        raise ValueError(f"Unknown descriptor: {name}")
    return PATCHDESC_MODELS[name]


def patchdesc_tensor_names(model: str) -> list[str]:
    lib, m = load_library(), patchdesc_model(model)
    return [lib.imcui_hip_patchdesc_tensor_name(m, i).decode() for i in range(lib.imcui_hip_patchdesc_num_tensors(m))]


def patchdesc_tensor_shapes(model: str) -> dict:
    root, shapes = PATCHDESC_ROOT[model], {}
    for (cin, cout, k), op in zip(PATCHDESC_LAYERS, PATCHDESC_CONV_OPS[model]):
        shapes[f"{root}.{op}.weight"] = (cout, cin, k, k)
        shapes[f"{root}.{op + 1}.running_mean"] = (cout,)
        shapes[f"{root}.{op + 1}.running_var"] = (cout,)
    return shapes


def _pack_patchdesc(model: str, state_dict: dict) -> torch.Tensor:
    lib = load_library()
    sd = dict(state_dict)
    if set(sd) >= {"state_dict"} and isinstance(sd["state_dict"], dict):  # HardNet's checkpoint_liberty_with_aug.pth wraps it
        sd = dict(sd["state_dict"])
    sd = {k: v for k, v in sd.items() if not k.endswith(".num_batches_tracked")}  # the counters of the affine-free BatchNorms
    return _pack_named(model, f"kornia's {'HardNet' if model == 'hardnet' else 'SOSNet'}", patchdesc_tensor_names(model), patchdesc_tensor_shapes(model), sd,
                       lib.imcui_hip_patchdesc_packed_floats(), lib.imcui_hip_patchdesc_pack_weights, patchdesc_model(model))  # fmt: skip


def pack_hardnet(state_dict: dict) -> torch.Tensor:
    """kornia.feature.HardNet's state dict (`features.N.*`, or a checkpoint {"state_dict": ...}) -> packed float32 buffer (host).
    Strict: every key but the `num_batches_tracked` counters is consumed exactly once, every shape checked."""
    return _pack_patchdesc("hardnet", state_dict)


def pack_sosnet(state_dict: dict) -> torch.Tensor:
    """kornia.feature.SOSNet's state dict (`layers.N.*`, or wrapped in {"state_dict": ...}) -> packed float32 buffer (host).  Strict."""
    return _pack_patchdesc("sosnet", state_dict)


def patchdesc_check_args(image_shape, kcap: int, chunk: int, mr_size: float) -> None:
    """Refusals raised before anything is launched (the library refuses the same)."""
    if len(image_shape) != 4 or image_shape[1] != 1:
        raise ValueError(f"the patch descriptors expect a gray image [B,1,H,W], got shape {tuple(image_shape)}")
    if image_shape[2] < 8 or image_shape[3] < 8:
        raise ValueError(f"the patch descriptors need images of at least 8 x 8, got {tuple(image_shape[2:])}")
    if kcap < 1 or not 1 <= chunk <= PATCHDESC_MAX_CHUNK:
        raise ValueError(f"kcap={kcap} must be positive and chunk={chunk} within 1..{PATCHDESC_MAX_CHUNK}")
    if not (mr_size > 0 and math.isfinite(mr_size)):
        raise ValueError(f"mr_size={mr_size} must be positive and finite")


class PatchDescHIP:
    """dog.py:87-105 on the device: LAF patches from the image pyramid, HardNet / SOSNet, unit descriptors (imcui_hip_patchdesc_forward)."""

    def __init__(self):
        self._ws = _Workspace()

    def forward(self, packed: torch.Tensor, image: torch.Tensor, keypoints: torch.Tensor, scales: torch.Tensor, oris_deg: torch.Tensor,
                num_keypoints: torch.Tensor, model: str, mr_size: float = 12.0, chunk: int = PATCHDESC_CHUNK, want_patches: bool = False,
                out: torch.Tensor | None = None) -> dict:  # fmt: skip
        """image [B,1,H,W] in [0,1]; keypoints [B,K,2] (x, y), scales [B,K] (sigma), oris_deg [B,K], num_keypoints [B] int32, all on the
        GPU -> {"descriptors": [B,K,128] (rows past num_keypoints[b] are not written: zero, or what `out` held), "status": [1] int32
        (bit 1: a count above K, bit 2: a non-finite key-point, its row is zero)}; want_patches adds "patches" [B,K,32,32].  No host
        synchronisation, graph-capturable."""
        m = patchdesc_model(model)
        B, K = keypoints.shape[:2]
        patchdesc_check_args(tuple(image.shape), K, chunk, float(mr_size))
        if image.shape[0] != B or tuple(keypoints.shape) != (B, K, 2) or tuple(scales.shape) != (B, K) or tuple(oris_deg.shape) != (B, K) or tuple(num_keypoints.shape) != (B,):
            raise ValueError(f"patch descriptors: image {tuple(image.shape)}, keypoints {tuple(keypoints.shape)}, scales {tuple(scales.shape)}, "
                             f"oris {tuple(oris_deg.shape)}, num_keypoints {tuple(num_keypoints.shape)} do not agree")  # fmt: skip
        hd = get_handle(image.device)
        _same_device(packed, image)
        lib = hd.lib
        if packed.numel() != lib.imcui_hip_patchdesc_packed_floats():
            raise ImcuiHipError(f"patch descriptors: the packed buffer holds {packed.numel()} floats, {lib.imcui_hip_patchdesc_packed_floats()} are needed")
        dev = image.device
        image, keypoints, scales, oris_deg = (t.contiguous().float() for t in (image, keypoints, scales, oris_deg))
        num_keypoints = num_keypoints.contiguous().to(torch.int32)
        _, _, H, W = image.shape
        desc = torch.zeros((B, K, 128), dtype=torch.float32, device=dev) if out is None else out
        if tuple(desc.shape) != (B, K, 128) or desc.dtype != torch.float32 or not desc.is_contiguous() or desc.device != dev:
            raise ValueError("patch descriptors: `out` must be a contiguous float32 [B,K,128] tensor on the image's device")
        status = torch.empty((1,), dtype=torch.int32, device=dev)
        patches = torch.zeros((B, K, 32, 32), dtype=torch.float32, device=dev) if want_patches else None
        nbytes = lib.imcui_hip_patchdesc_workspace_bytes(B, H, W, K, int(chunk))
        if nbytes == 0:
            raise ImcuiHipError(f"patch descriptors: unsupported launch (B={B}, {H}x{W}, K={K}, chunk={chunk})")
        with self._ws.use(nbytes, dev) as ws:
            hd.launch(lib.imcui_hip_patchdesc_forward, _ptr(packed), _ptr(image), B, H, W, _ptr(keypoints), _ptr(scales), _ptr(oris_deg), _ptr(num_keypoints), K, m,
                      float(mr_size), int(chunk), _ptr(desc), _ptr(status), _ptr(patches), _ptr(ws), ws.numel())  # fmt: skip
        res = {"descriptors": desc, "status": status}
        if want_patches:
            res["patches"] = patches
        return res

    def layer_probe(self, op: str, inp: torch.Tensor, model: str = "hardnet", packed: torch.Tensor | None = None) -> torch.Tensor:
        """Test entry: one launch alone, as the forward makes it.  "pyrdown": [n,H,W] -> [n,H//2,W//2]; "norm": patches [n,32,32] -> the
        network's input normalisation; "layer1": patches -> NHWC [n,32,32,32]; "layer2" .. "layer6": NHWC in -> NHWC out; "final":
        [n,8,8,128] -> [n,128] (BatchNorm folded, not normalised); "outnorm": [n,128] -> [n,128].  All but pyrdown / norm / outnorm need `packed`."""
        code, m = PATCHDESC_PROBE_OPS[op], patchdesc_model(model)
        hd = get_handle(inp.device)
        lib = hd.lib
        inp = inp.contiguous().float()
        n, H, W = inp.shape[0], 1, 1
        if code == 0:
            _, H, W = inp.shape
            shape = (n, H // 2, W // 2)
        elif code == 1:
            shape = tuple(inp.shape)
        elif code == 2:
            shape = (n, 32, 32, 32)
        elif code <= 7:
            cin, cout, _ = PATCHDESC_LAYERS[code - 2]
            hin, hout = (32, 32, 16, 16, 8)[code - 3], (32, 16, 16, 8, 8)[code - 3]
            if tuple(inp.shape) != (n, hin, hin, cin):
                raise ValueError(f"{op}: expected NHWC [{n},{hin},{hin},{cin}], got {tuple(inp.shape)}")
            shape = (n, hout, hout, cout)
        else:
            shape = (n, 128)
        if code in (1, 2) and inp[0].numel() != 1024 or code == 8 and inp[0].numel() != 8192 or code == 9 and inp[0].numel() != 128:
            raise ValueError(f"{op}: input of shape {tuple(inp.shape)}")
        out = torch.empty(shape, dtype=torch.float32, device=inp.device)
        with self._ws.use(lib.imcui_hip_patchdesc_probe_workspace_bytes(n, H, W), inp.device) as ws:
            hd.launch(lib.imcui_hip_patchdesc_layer_probe, code, m, _ptr(packed), _ptr(inp), n, H, W, _ptr(out), _ptr(ws), ws.numel())
        return out

    def patch_probe(self, image: torch.Tensor, keypoints: torch.Tensor, scales: torch.Tensor, oris_deg: torch.Tensor, mr_size: float = 12.0):
        """Test entry: pyramid + sampling alone on ONE image [H,W]: keypoints [n,2], scales [n], oris_deg [n] -> (patches [n,32,32], status [1])."""
        hd = get_handle(image.device)
        lib = hd.lib
        image, keypoints, scales, oris_deg = (t.contiguous().float() for t in (image, keypoints, scales, oris_deg))
        (H, W), n = image.shape, keypoints.shape[0]
        patches = torch.empty((n, 32, 32), dtype=torch.float32, device=image.device)
        status = torch.empty((1,), dtype=torch.int32, device=image.device)
        nbytes = lib.imcui_hip_patchdesc_patch_probe_workspace_bytes(H, W)
        if nbytes == 0:
            raise ImcuiHipError(f"patch probe: unsupported image {H}x{W}")
        with self._ws.use(nbytes, image.device) as ws:
            hd.launch(lib.imcui_hip_patchdesc_patch_probe, _ptr(image), H, W, _ptr(keypoints), _ptr(scales), _ptr(oris_deg), n, float(mr_size), _ptr(patches),
                      _ptr(status), _ptr(ws), ws.numel())  # fmt: skip
        return patches, status


# ------------------------------------------------------------------ SIFT
SIFT_LAYERS =(3, 4, 5)  # nOctaveLayers (the wrapper's `num_octaves`) csrc/sift.hip is written for: blur radius at most 13


def sift_check_args(image_shape, conf: dict) -> None:
    """Refusals raised before anything is launched (imcui/hloc/extractors/sift.py: backend "opencv" only)."""
    if len(image_shape) != 4 or image_shape[1] not in (1, 3):
        raise ValueError(f"SIFT expects an image [B,1,H,W] or [B,3,H,W], got shape {tuple(image_shape)}")
    if image_shape[2] < 8 or image_shape[3] < 8:
        raise ValueError(f"SIFT needs images of at least 8 x 8, got {tuple(image_shape[2:])}")
    backend_name = str(conf.get("backend", "opencv"))
    if backend_name.startswith("pycolmap"):
        raise ImcuiHipError(f"SIFT backend '{backend_name}' is not served by the HIP backend: only `opencv` (the default, and what `sift` / `sift-lightglue` use)")
    if backend_name != "opencv":
        raise ValueError(f"Unknown backend: {backend_name} not in {{opencv,pycolmap,pycolmap_cpu,pycolmap_cuda}}.")
    if conf.get("first_octave", -1) != -1:
        raise ImcuiHipError("SIFT `first_octave` is only read by the pycolmap backends (ignored by `opencv`): leave it at its default -1")
    if int(conf["num_octaves"]) not in SIFT_LAYERS:
        raise ImcuiHipError(f"SIFT num_octaves={conf['num_octaves']} (passed to OpenCV as nOctaveLayers) is outside what the HIP kernels serve: {SIFT_LAYERS}")
    r = conf.get("nms_radius")
    if r is not None and not 0 <= int(r) <= 64:
        raise ValueError(f"nms_radius={r} is outside 0..64 (None skips the filter)")


def sift_octave_shapes(H: int, W: int) -> list[tuple[int, int]]:
    """(h, w) of every octave of an H x W image (octave 0 is the doubled image)."""
    n = load_library().imcui_hip_sift_num_octaves(H, W)
    out, h, w = [], 2 * H, 2 * W
    for _ in range(n):
        if h < 1 or w < 1:
            break
        out.append((h, w))
        h, w = h // 2, w // 2
    return out


class SiftHIP:
    def __init__(self):
        self._ws = _Workspace()

    @staticmethod
    def default_ccap(H: int, W: int) -> int:
        """Room for the extrema of an image: a quarter of its pixels (structured images have 5-10 %); `forward_checked` retries."""
        return max(1024, H * W // 4)

    def forward(self, image: torch.Tensor, conf: dict, kcap: int | None = None, ccap: int | None = None, debug: bool = False):
        """image [B,1|3,H,W] float in [0,1] on the GPU -> fixed-stride outputs, no host synchronisation: keypoints [B,K,2], scores,
        scales, oris [B,K], descriptors [B,K,128], num_keypoints [B] int32, status [1] int32 (bit 1: `kcap` too small, bit 2: `ccap` too
        small), counts [B,3] int32 (extrema, oriented key-points, survivors: unclipped).  debug adds pyramid (list per octave of
        [B,layers+3,h,w] views), extrema, refined, hist, table, desc_raw."""
        sift_check_args(tuple(image.shape), conf)
        hd = get_handle(image.device)
        lib = hd.lib
        image = image.contiguous().float()
        B, C, H, W = image.shape
        layers = int(conf["num_octaves"])
        maxk = conf.get("max_keypoints")
        maxk = int(maxk) if maxk is not None and int(maxk) > 0 else 0
        r = conf.get("nms_radius")
        r = -1 if r is None else int(r)
        if ccap is None:
            ccap = self.default_ccap(H, W)
        if kcap is None:
            kcap = min(maxk, ccap) if maxk else ccap
        ccap = int(ccap)
        kcap = max(1, min(int(kcap), ccap))
        nbytes = lib.imcui_hip_sift_workspace_bytes(B, H, W, layers, ccap, kcap)
        if nbytes == 0:
            raise ImcuiHipError(f"SIFT: unsupported launch (B={B}, {H}x{W}, layers={layers}, ccap={ccap}, kcap={kcap})")
        dev = image.device
        f32, i32 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
        kpts = torch.empty((B, kcap, 2), **f32)
        scores, scales, oris = (torch.empty((B, kcap), **f32) for _ in range(3))
        desc = torch.empty((B, kcap, 128), **f32)
        nk, status, counts = torch.empty((B,), **i32), torch.empty((1,), **i32), torch.empty((B, 3), **i32)
        dbg = {}
        if debug:
            dbg = dict(pyramid=torch.empty((lib.imcui_hip_sift_pyramid_floats(B, H, W, layers),), **f32), extrema=torch.empty((B, ccap), **i32),
                       refined=torch.empty((B, ccap, 16), **f32), hist=torch.empty((B, ccap, 36), **f32), table=torch.empty((B, ccap, 12), **f32),
                       desc_raw=torch.empty((B, kcap, 128), **f32))  # fmt: skip
        with self._ws.use(nbytes, dev) as ws:
            hd.launch(
                lib.imcui_hip_sift_forward, _ptr(image), B, C, H, W, layers, float(conf["detection_threshold"]), float(conf["edge_threshold"]), maxk, r, maxk,
                int(bool(conf["rootsift"])), ccap, kcap, _ptr(kpts), _ptr(scores), _ptr(scales), _ptr(oris), _ptr(desc), _ptr(nk), _ptr(status), _ptr(counts),
                _ptr(dbg.get("pyramid")), _ptr(dbg.get("extrema")), _ptr(dbg.get("refined")), _ptr(dbg.get("hist")), _ptr(dbg.get("table")),
                _ptr(dbg.get("desc_raw")), _ptr(ws), ws.numel(),
            )  # fmt: skip
        out = {"keypoints": kpts, "scores": scores, "scales": scales, "oris": oris, "descriptors": desc, "num_keypoints": nk, "status": status, "counts": counts}
        if debug:
            flat, off, pyr = dbg.pop("pyramid"), 0, []
            for h, w in sift_octave_shapes(H, W):
                n = B * (layers + 3) * h * w
                pyr.append(flat[off : off + n].view(B, layers + 3, h, w))
                off += n
            out.update(dbg, pyramid=pyr)
        return out


# ------------------------------------------------------------------ LightGlue
def lightglue_tensor_names() -> list[str]:
    lib = load_library()
    return [lib.imcui_hip_lightglue_tensor_name(i).decode() for i in range(lib.imcui_hip_lightglue_num_tensors())]


def _rename_old_lightglue_keys(sd: dict) -> dict:
    """Old checkpoints name blocks `self_attn.{i}...` / `cross_attn.{i}...` (renamed on load upstream)."""
    out = {}
    for k, v in sd.items():
        for i in range(9):
            for blk in ("self_attn", "cross_attn"):
                old = f"{blk}.{i}"
                if k.startswith(old + "."):
                    k = f"transformers.{i}.{blk}" + k[len(old):]
        out[k] = v
    return out


def lightglue_variant(state_dict: dict) -> tuple[int, bool]:
    """(input_dim, add_scale_ori) of a LightGlue state dict: upstream's `features` table in the weights themselves --
    `input_proj` exists when the descriptors are not 256-d (disk / aliked / sift: 128), `posenc.Wr` has 4 input columns
    when key-point scale and orientation are encoded (sift, doghardnet)."""
    sd = _rename_old_lightglue_keys(state_dict)
    input_dim = int(sd["input_proj.weight"].shape[1]) if "input_proj.weight" in sd else 256
    return input_dim, int(sd["posenc.Wr.weight"].shape[1]) == 4


def pack_lightglue(state_dict: dict) -> torch.Tensor:
    lib = load_library()
    sd = _rename_old_lightglue_keys(state_dict)
    names = lightglue_tensor_names()
    arrs = []
    for n in names:
        if n not in sd:
            raise ImcuiHipError(f"LightGlue state dict lacks '{n}'")
        arrs.append(_as_f32_host(sd[n]))
    input_dim, scale_ori = lightglue_variant(sd)
    if arrs[0].shape not in ((32, 2), (32, 4)) or arrs[1].shape != (768, 256) or input_dim % 32 or input_dim > 256:
        raise ImcuiHipError("only the 256-d / 4-head / 9-layer LightGlue (descriptor input 32..256, optional scale / orientation) is supported")
    packed = np.zeros(lib.imcui_hip_lightglue_packed_floats(), dtype=np.float32)
    wr = arrs[0]
    arrs[0] = np.ascontiguousarray(wr[:, :2])  # the base packer takes the (x, y) columns; pack_input stores all of them
    tp = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
    rc = lib.imcui_hip_lightglue_pack_weights(tp, packed.ctypes.data)
    if rc != 0:
        raise ImcuiHipError(f"imcui_hip_lightglue_pack_weights failed ({rc})")
    wi = _as_f32_host(sd["input_proj.weight"]) if input_dim != 256 else None
    bi = _as_f32_host(sd["input_proj.bias"]) if input_dim != 256 else None
    rc = lib.imcui_hip_lightglue_pack_input(wr.ctypes.data, wr.shape[1], None if wi is None else wi.ctypes.data,
                                            None if bi is None else bi.ctypes.data, input_dim, packed.ctypes.data)  # fmt: skip
    if rc != 0:
        raise ImcuiHipError(f"imcui_hip_lightglue_pack_input failed ({rc})")
    return torch.from_numpy(packed)


class LightGlueHIP:
    def __init__(self):
        self._ws = _Workspace()

    def forward(self, packed, kpts0, kpts1, desc0, desc1, n0, n1, size0, size1, depth_confidence, width_confidence,
                filter_threshold, pruning_threshold: int = -1, layer_dump: bool = False, scales_oris=None):  # fmt: skip
        """kptsX [B,ncap,2], descX [B,ncap,D] (row per point; D = the weights' input_dim), nX [B] int32 on the GPU;
        sizeX = (W, H); scales_oris = (scales0, oris0, scales1, oris1) [B,ncap] for add_scale_ori weights.
        pruning_threshold: upstream pruning_keypoint_thresholds[device] (-1 = the CPU path: always prune).
        layer_dump (parity tests): also return `_layers` [9, 2B, R, 256], the token states after every layer."""
        dev = kpts0.device
        hd = get_handle(dev)
        lib = hd.lib
        B, ncap0 = kpts0.shape[0], kpts0.shape[1]
        ncap1 = kpts1.shape[1]
        ncap = max(ncap0, ncap1, 1)
        kpts0, kpts1, desc0, desc1 = (_pad_rows(t, ncap, dev) for t in (kpts0, kpts1, desc0, desc1))
        input_dim = desc0.shape[2]
        so = [None] * 4 if scales_oris is None else [_pad_rows(t, ncap, dev) for t in scales_oris]
        n0 = n0.to(device=dev, dtype=torch.int32).contiguous()
        n1 = n1.to(device=dev, dtype=torch.int32).contiguous()
        m0 = torch.empty((B, ncap), dtype=torch.int32, device=dev)
        m1 = torch.empty((B, ncap), dtype=torch.int32, device=dev)
        s0 = torch.empty((B, ncap), dtype=torch.float32, device=dev)
        s1 = torch.empty((B, ncap), dtype=torch.float32, device=dev)
        stop = torch.empty((B,), dtype=torch.int32, device=dev)
        p0 = torch.empty((B, ncap), dtype=torch.int32, device=dev)
        p1 = torch.empty((B, ncap), dtype=torch.int32, device=dev)
        dump = None
        with self._ws.use(lib.imcui_hip_lightglue_workspace_bytes(B, ncap), dev) as ws:
            if layer_dump:
                R = (ncap + 127) // 128 * 128
                dump = torch.zeros((9, 2 * B, R, 256), dtype=torch.float32, device=dev)
                hd.call(lib.imcui_hip_lightglue_set_layer_dump, _ptr(dump), dump.numel())
            try:
                hd.launch(
                    lib.imcui_hip_lightglue_forward, _ptr(packed), B, ncap, input_dim, _ptr(kpts0), _ptr(kpts1), _ptr(desc0), _ptr(desc1),
                    _ptr(so[0]), _ptr(so[1]), _ptr(so[2]), _ptr(so[3]), _ptr(n0), _ptr(n1),
                    float(size0[0]), float(size0[1]), float(size1[0]), float(size1[1]),
                    float(depth_confidence), float(width_confidence), int(pruning_threshold), float(filter_threshold),
                    _ptr(m0), _ptr(m1), _ptr(s0), _ptr(s1), _ptr(stop), _ptr(p0), _ptr(p1), _ptr(ws), ws.numel(),
                )  # fmt: skip
            finally:
                if layer_dump:
                    lib.imcui_hip_lightglue_set_layer_dump(hd.h, None, 0)
        out = {
            "matches0": m0[:, :ncap0], "matches1": m1[:, :ncap1], "matching_scores0": s0[:, :ncap0],
            "matching_scores1": s1[:, :ncap1], "stop": stop, "prune0": p0[:, :ncap0], "prune1": p1[:, :ncap1],
        }  # fmt: skip
        if dump is not None:
            out["_layers"] = dump
        return out


# ------------------------------------------------------------------ SuperGlue
def superglue_tensor_names() -> list[str]:
    lib = load_library()
    return [lib.imcui_hip_superglue_tensor_name(i).decode() for i in range(lib.imcui_hip_superglue_num_tensors())]


def pack_superglue(state_dict: dict) -> torch.Tensor:
    """Upstream SuperGlue state dict (Conv1d weights [out,in,1]) -> packed float32 buffer (host)."""
    lib = load_library()
    names = superglue_tensor_names()
    arrs = []
    for n in names:
        if n not in state_dict:
            raise ImcuiHipError(f"SuperGlue state dict lacks '{n}'")
        arrs.append(_as_f32_host(state_dict[n]).reshape(-1) if n == "bin_score" else _as_f32_host(state_dict[n]))
    if arrs[0].size != 32 * 3 or arrs[names.index("gnn.layers.17.mlp.3.weight")].size != 256 * 512:
        raise ImcuiHipError("only the 256-d / 4-head / 18-layer SuperGlue with the [32,64,128,256] key-point encoder is supported")
    return _pack_arrays(arrs, lib.imcui_hip_superglue_packed_floats(), lib.imcui_hip_superglue_pack_weights)


def _glue_forward(wsp, ws_bytes_fn: str, forward_fn: str, packed, kpts0, kpts1, scores0, scores1, desc0, desc1, n0, n1, size0, size1,
                  sinkhorn_iterations, match_threshold) -> dict:  # fmt: skip
    """The forward of the matchers on the SuperGlue trunk (SuperGlueHIP, IMPHIP), which differ in the two library entries named here:
    pads both sides to one ncap, runs in the workspace `wsp`, returns matches / scores cut back to each side's own length."""
    dev = kpts0.device
    hd = get_handle(dev)
    lib = hd.lib
    B, ncap0 = kpts0.shape[0], kpts0.shape[1]
    ncap1 = kpts1.shape[1]
    ncap = max(ncap0, ncap1, 1)
    kpts0, kpts1, desc0, desc1, scores0, scores1 = (_pad_rows(t, ncap, dev) for t in (kpts0, kpts1, desc0, desc1, scores0, scores1))
    n0 = n0.to(device=dev, dtype=torch.int32).contiguous()
    n1 = n1.to(device=dev, dtype=torch.int32).contiguous()
    m0 = torch.empty((B, ncap), dtype=torch.int32, device=dev)
    m1 = torch.empty((B, ncap), dtype=torch.int32, device=dev)
    s0 = torch.empty((B, ncap), dtype=torch.float32, device=dev)
    s1 = torch.empty((B, ncap), dtype=torch.float32, device=dev)
    with wsp.use(getattr(lib, ws_bytes_fn)(B, ncap), dev) as ws:
        hd.launch(
            getattr(lib, forward_fn), _ptr(packed), B, ncap, _ptr(kpts0), _ptr(kpts1), _ptr(scores0), _ptr(scores1), _ptr(desc0), _ptr(desc1),
            _ptr(n0), _ptr(n1), float(size0[0]), float(size0[1]), float(size1[0]), float(size1[1]),
            int(sinkhorn_iterations), float(match_threshold),
            _ptr(m0), _ptr(m1), _ptr(s0), _ptr(s1), _ptr(ws), ws.numel(),
        )  # fmt: skip
    return {
        "matches0": m0[:, :ncap0], "matches1": m1[:, :ncap1], "matching_scores0": s0[:, :ncap0],
        "matching_scores1": s1[:, :ncap1],
    }  # fmt: skip


class SuperGlueHIP:
    def __init__(self):
        self._ws = _Workspace()

    def forward(self, packed, kpts0, kpts1, scores0, scores1, desc0, desc1, n0, n1, size0, size1, sinkhorn_iterations,
                match_threshold):  # fmt: skip
        """kptsX [B,ncap,2], scoresX [B,ncap], descX [B,ncap,256] (row per point), nX [B] int32 on the GPU; sizeX = (W, H)."""
        return _glue_forward(self._ws, "imcui_hip_superglue_workspace_bytes", "imcui_hip_superglue_forward", packed, kpts0, kpts1, scores0, scores1,
                             desc0, desc1, n0, n1, size0, size1, sinkhorn_iterations, match_threshold)  # fmt: skip


# ------------------------------------------------------------------ IMP
def imp_tensor_table() -> list[tuple[str, tuple]]:
    """(state-dict name, shape) of every tensor of `imp_gml.920.pth`, from the one table generator in csrc/glue_shared.h."""
    lib = load_library()
    dims = (C.c_int * 3)()
    out = []
    for i in range(lib.imcui_hip_imp_num_tensors()):
        nd = lib.imcui_hip_imp_tensor_shape(i, dims)
        out.append((lib.imcui_hip_imp_tensor_name(i).decode(), tuple(dims[:nd])))
    return out


def pack_imp(state_dict: dict, conf: dict | None = None) -> torch.Tensor:
    """pram.nets.gml.GML state dict -> packed float32 buffer (host).  Strict, like the reference's `load_state_dict(..., strict=True)`
    (imcui/hloc/matchers/imp.py:41-44): a missing name, a shape that differs or an extra key is refused with a message that names it."""
    conf = conf or {}
    name = str(conf.get("model_name", ""))
    if "adagml" in name.lower() or any(k.startswith(("pooling", "pool.", "ada")) for k in state_dict):
        raise ImcuiHipError(f"IMP: the adaptive-pooling model (AdaGML, '{name or 'imp_adagml*'}') is not built; only GML (imp_gml*) runs here")
    if conf.get("with_sinkhorn", True) is False:
        raise ImcuiHipError("IMP: with_sinkhorn=False (the dual-softmax score) is not built; only the Sinkhorn assignment runs here")
    if int(conf.get("n_layers", 9)) != 9:
        raise ImcuiHipError(f"IMP: n_layers={conf['n_layers']} is not built; only the 9 x ['self', 'cross'] network runs here")
    lib = load_library()
    table = imp_tensor_table()
    w = state_dict.get("input_proj.weight")
    if w is not None and tuple(w.shape)[:2] != (256, 128):
        raise ImcuiHipError(f"IMP: input_proj takes {tuple(w.shape)[1]}-wide descriptors; only the 128-wide (sfd2) model runs here")
    bn = {n[: -len("running_var")] + "num_batches_tracked" for n, _ in table if n.endswith(".running_var")}  # BatchNorm's counter, not a weight
    extra = sorted(set(state_dict) - {n for n, _ in table} - bn)
    if extra:
        raise ImcuiHipError(f"IMP: the state dict has {len(extra)} keys the network does not: {', '.join(extra[:8])}{' ...' if len(extra) > 8 else ''}")
    arrs = []
    for n, shp in table:
        if n not in state_dict:
            raise ImcuiHipError(f"IMP state dict lacks '{n}'")
        if tuple(state_dict[n].shape) != shp:
            raise ImcuiHipError(f"IMP: '{n}' has shape {tuple(state_dict[n].shape)}, the network needs {shp}")
        arrs.append(_as_f32_host(state_dict[n]).reshape(-1) if not shp else _as_f32_host(state_dict[n]))
    return _pack_arrays(arrs, lib.imcui_hip_imp_packed_floats(), lib.imcui_hip_imp_pack_weights)


class IMPHIP:
    def __init__(self):
        self._ws = _Workspace()

    def forward(self, packed, kpts0, kpts1, scores0, scores1, desc0, desc1, n0, n1, size0, size1, sinkhorn_iterations,
                match_threshold):  # fmt: skip
        """kptsX [B,ncap,2], scoresX [B,ncap], descX [B,ncap,128] (row per point), nX [B] int32 on the GPU; sizeX = (W, H)."""
        return _glue_forward(self._ws, "imcui_hip_imp_workspace_bytes", "imcui_hip_imp_forward", packed, kpts0, kpts1, scores0, scores1,
                             desc0, desc1, n0, n1, size0, size1, sinkhorn_iterations, match_threshold)  # fmt: skip

    def ot_probe(self, scores, n0, n1, bin_score, iterations, p=0.2) -> dict:
        """The assignment stage alone (imcui_hip_imp_ot_probe): scores [B,ncap,ncap] float32 on the GPU, n0 / n1 [B] int32.
        u / v [B,ncap+1]: entry n0[b] / n1[b] is the dust-bin's."""
        dev = scores.device
        hd = get_handle(dev)
        lib = hd.lib
        B, ncap = scores.shape[0], scores.shape[1]
        assert scores.shape[2] == ncap and scores.dtype == torch.float32
        scores = scores.contiguous()
        n0 = n0.to(device=dev, dtype=torch.int32).contiguous()
        n1 = n1.to(device=dev, dtype=torch.int32).contiguous()
        m0 = torch.empty((B, ncap), dtype=torch.int32, device=dev)
        m1 = torch.empty((B, ncap), dtype=torch.int32, device=dev)
        s0 = torch.empty((B, ncap), dtype=torch.float32, device=dev)
        s1 = torch.empty((B, ncap), dtype=torch.float32, device=dev)
        u = torch.empty((B, ncap + 1), dtype=torch.float32, device=dev)
        v = torch.empty((B, ncap + 1), dtype=torch.float32, device=dev)
        with self._ws.use(lib.imcui_hip_imp_workspace_bytes(B, ncap), dev) as ws:
            hd.launch(
                lib.imcui_hip_imp_ot_probe, _ptr(scores), B, ncap, _ptr(n0), _ptr(n1), float(bin_score), int(iterations), float(p),
                _ptr(m0), _ptr(m1), _ptr(s0), _ptr(s1), _ptr(u), _ptr(v), _ptr(ws), ws.numel(),
            )  # fmt: skip
        return {"matches0": m0, "matches1": m1, "matching_scores0": s0, "matching_scores1": s1, "u": u, "v": v}


# ------------------------------------------------------------------ AdaLAM
ADALAM_CONF_KEYS = ("area_ratio", "search_expansion", "ransac_iters", "min_inliers", "min_confidence", "orientation_difference_threshold",
                    "scale_rate_threshold", "detected_scale_rate_threshold", "refit", "force_seed_mnn")  # the order of the C ABI's conf array
ADALAM_MAX_KEYPOINTS = 4096  # AL_MAXN of csrc/adalam.hip
ADALAM_WIDTHS = (64, 128, 256)


def adalam_conf_array(conf: dict):
    """The conf as the C ABI takes it: 10 doubles in ADALAM_CONF_KEYS order, None (a threshold that is off) as -1."""
    vals = []
    for k in ADALAM_CONF_KEYS:
        v = conf[k]
        if v is None:
            if not k.endswith("_threshold"):
                raise ImcuiHipError(f"AdaLAM: conf['{k}'] is None")
            v = -1.0
        elif k.endswith("_threshold") and float(v) < 0:
            raise ImcuiHipError(f"AdaLAM: conf['{k}'] = {v} (a threshold is None or >= 0)")
        vals.append(float(v))
    return (C.c_double * len(vals))(*vals)


def adalam_needs(conf: dict) -> tuple:
    """(orientations needed, scales needed): whether the two relative tests are on (kornia: off at None, or at >= 180 / >= 10)."""
    ot, st = conf["orientation_difference_threshold"], conf["scale_rate_threshold"]
    return ot is not None and float(ot) < 180.0, st is not None and float(st) < 10.0


class AdaLAMHIP:
    def __init__(self):
        self._ws = _Workspace()

    def _run(self, desc, nn_in, kpts0, kpts1, n0, n1, size0, size1, conf, scales_oris, probe, members):
        dev = kpts0.device
        hd = get_handle(dev)
        lib = hd.lib
        B, ncap = kpts0.shape[0], max(kpts0.shape[1], kpts1.shape[1], 1)
        if ncap > ADALAM_MAX_KEYPOINTS:
            raise ImcuiHipError(f"AdaLAM: {ncap} key-points per image, the kernels take at most {ADALAM_MAX_KEYPOINTS}")
        carr = adalam_conf_array(conf)
        need_o, need_s = adalam_needs(conf)
        s0, o0, s1, o1 = (None,) * 4 if scales_oris is None else scales_oris
        if need_o and (o0 is None or o1 is None):
            raise ImcuiHipError("AdaLAM: orientation_difference_threshold is active but oris0 / oris1 are missing")
        if need_s and (s0 is None or s1 is None):
            raise ImcuiHipError("AdaLAM: scale_rate_threshold is active but scales0 / scales1 are missing")
        k0, k1 = _pad_rows(kpts0, ncap, dev), _pad_rows(kpts1, ncap, dev)
        so = [None if t is None else _pad_rows(t, ncap, dev) for t in (s0, s1, o0, o1)]
        n0 = n0.to(device=dev, dtype=torch.int32).contiguous()
        n1 = n1.to(device=dev, dtype=torch.int32).contiguous()
        (w0, h0), (w1, h1) = size0, size1
        m0 = torch.empty((B, ncap), dtype=torch.int32, device=dev)
        ms0 = torch.empty((B, ncap), dtype=torch.float32, device=dev)
        out = {"matches0": m0, "matching_scores0": ms0}
        opt = {}
        if probe:
            opt = {"seed": torch.empty((B, ncap), dtype=torch.int32, device=dev), "seed_info": torch.empty((B, ncap, 4), dtype=torch.int32, device=dev),
                   "seed_conf": torch.empty((B, ncap), dtype=torch.float32, device=dev)}  # fmt: skip
            if members:
                opt["seed_members"] = torch.full((B, ncap, ncap), -1, dtype=torch.int32, device=dev)
        tail = (_ptr(opt.get("seed")), _ptr(opt.get("seed_members")), _ptr(opt.get("seed_info")), _ptr(opt.get("seed_conf")))
        geom = (_ptr(k0), _ptr(k1), _ptr(so[0]), _ptr(so[1]), _ptr(so[2]), _ptr(so[3]), _ptr(n0), _ptr(n1), int(h0), int(w0), int(h1), int(w1), carr)
        if desc is not None:
            d0, d1 = desc
            D = d0.shape[2]
            if D not in ADALAM_WIDTHS or d1.shape[2] != D:
                raise ImcuiHipError(f"AdaLAM: descriptor width {D} / {d1.shape[2]}, the kernels take {ADALAM_WIDTHS}")
            d0, d1 = _pad_rows(d0, ncap, dev), _pad_rows(d1, ncap, dev)
            if probe:
                opt.update(nn=torch.empty((B, ncap), dtype=torch.int32, device=dev), score=torch.empty((B, ncap), dtype=torch.float32, device=dev),
                           mnn=torch.empty((B, ncap), dtype=torch.int32, device=dev))  # fmt: skip
            with self._ws.use(max(256, lib.imcui_hip_adalam_workspace_bytes(hd.h, B, ncap, D)), dev) as ws:
                hd.launch(lib.imcui_hip_adalam_forward, B, ncap, D, _ptr(d0), _ptr(d1), *geom, _ptr(m0), _ptr(ms0), _ptr(opt.get("nn")),
                          _ptr(opt.get("score")), _ptr(opt.get("mnn")), *tail, _ptr(ws), ws.numel())  # fmt: skip
        else:
            nn, score, mnn = nn_in
            nn, score, mnn = _pad_rows(nn, ncap, dev).to(torch.int32), _pad_rows(score, ncap, dev), _pad_rows(mnn, ncap, dev).to(torch.int32)
            with self._ws.use(max(256, lib.imcui_hip_adalam_workspace_bytes(hd.h, B, ncap, 0)), dev) as ws:
                hd.launch(lib.imcui_hip_adalam_filter, B, ncap, *geom, _ptr(nn), _ptr(score), _ptr(mnn), _ptr(m0), _ptr(ms0), *tail, _ptr(ws), ws.numel())
        out.update(opt)
        return out

    def forward(self, kpts0, kpts1, desc0, desc1, n0, n1, size0, size1, conf, scales_oris=None, probe: bool = False, members: bool = False) -> dict:
        """kptsX [B,ncap,2], descX [B,ncap,D] (row per point, D in ADALAM_WIDTHS), nX [B] int32 on the GPU; sizeX = (W, H); scales_oris =
        (scales0, oris0, scales1, oris1) [B,ncap] or None; conf = the plugin's.  probe: also nn / score / mnn, seed, seed_info [B,ncap,4]
        {members, best iteration, count, passed}, seed_conf; members: also seed_members [B,ncap,ncap].  No host synchronisation."""
        return self._run((desc0, desc1), None, kpts0, kpts1, n0, n1, size0, size1, conf, scales_oris, probe, members)

    def filter(self, kpts0, kpts1, nn, score, mnn, n0, n1, size0, size1, conf, scales_oris=None, probe: bool = True, members: bool = False) -> dict:
        """Stages B .. G (imcui_hip_adalam_filter) from given nn [B,ncap] int, score [B,ncap] float32, mnn [B,ncap] 0 / 1."""
        return self._run(None, (nn, score, mnn), kpts0, kpts1, n0, n1, size0, size1, conf, scales_oris, probe, members)


# ------------------------------------------------------------------ LoFTR
def _fold_bn(w: torch.Tensor, sd: dict, bn: str | None, eps: float = 1e-5):
    """conv (no bias) followed by eval-mode BatchNorm -> (w', b')."""
    cout = w.shape[0]
    if bn is None:
        return w, torch.zeros(cout)
    g = sd[bn + ".weight"].float() / torch.sqrt(sd[bn + ".running_var"].float() + eps)
    return w * g.view(-1, 1, 1, 1), sd[bn + ".bias"].float() - sd[bn + ".running_mean"].float() * g


def _conv_gemm_layout(w: torch.Tensor, b: torch.Tensor, n_pad: int, cin_pad: int):
    """OIHW -> [Cout_pad][tap][Cin_pad] (K order of the implicit im2col), zero padded."""
    cout, cin, kh, kw = w.shape
    out = torch.zeros(n_pad, kh * kw, cin_pad)
    out[:cout, :, :cin] = w.permute(0, 2, 3, 1).reshape(cout, kh * kw, cin)
    bo = torch.zeros(n_pad)
    bo[:cout] = b
    return out.reshape(n_pad, kh * kw * cin_pad).contiguous(), bo


def pack_loftr(state_dict: dict) -> torch.Tensor:
    """kornia LoFTR state dict -> packed float32 buffer (host): BN folding, GEMM layouts, 196 -> 256 padding."""
    lib = load_library()
    sd = {k: v.detach().float().cpu() for k, v in state_dict.items() if isinstance(v, torch.Tensor)}
    bb = "backbone."
    w1, b1 = _fold_bn(sd[bb + "conv1.weight"], sd, bb + "bn1")
    conv1_w = w1[:, 0].reshape(128, 49).t().contiguous().numpy()  # [tap][cout]
    conv1_b = b1.contiguous().numpy()
    P = lambda c: 256 if c == 196 else c  # noqa: E731
    convs = [  # (weight key, bn key or None) in the order of the C layer table
        ("layer1.0.conv1", "layer1.0.bn1"), ("layer1.0.conv2", "layer1.0.bn2"), ("layer1.1.conv1", "layer1.1.bn1"), ("layer1.1.conv2", "layer1.1.bn2"),
        ("layer2.0.conv1", "layer2.0.bn1"), ("layer2.0.conv2", "layer2.0.bn2"), ("layer2.0.downsample.0", "layer2.0.downsample.1"),
        ("layer2.1.conv1", "layer2.1.bn1"), ("layer2.1.conv2", "layer2.1.bn2"),
        ("layer3.0.conv1", "layer3.0.bn1"), ("layer3.0.conv2", "layer3.0.bn2"), ("layer3.0.downsample.0", "layer3.0.downsample.1"),
        ("layer3.1.conv1", "layer3.1.bn1"), ("layer3.1.conv2", "layer3.1.bn2"),
        ("layer3_outconv", None), ("layer2_outconv", None), ("layer2_outconv2.0", "layer2_outconv2.1"), ("layer2_outconv2.3", None),
        ("layer1_outconv", None), ("layer1_outconv2.0", "layer1_outconv2.1"), ("layer1_outconv2.3", None),
    ]  # fmt: skip
    ws, bs = [], []
    for wk, bk in convs:
        w, b = _fold_bn(sd[bb + wk + ".weight"], sd, bb + bk if bk else None)
        wg, bg = _conv_gemm_layout(w, b, P(w.shape[0]), P(w.shape[1]))
        ws.append(wg)
        bs.append(bg)
    lin_names = ["q_proj", "k_proj", "v_proj", "merge", "mlp.0", "mlp.2"]
    for i in range(8):
        for n in lin_names:
            ws.append(sd[f"loftr_coarse.layers.{i}.{n}.weight"].contiguous())
            bs.append(None)
    for n in ("down_proj", "merge_feat"):
        ws.append(sd[f"fine_preprocess.{n}.weight"].contiguous())
        bs.append(sd[f"fine_preprocess.{n}.bias"].contiguous())
    for i in range(2):
        for n in lin_names:
            ws.append(sd[f"loftr_fine.layers.{i}.{n}.weight"].contiguous())
            bs.append(None)
    norms = []
    for pre, nl in (("loftr_coarse", 8), ("loftr_fine", 2)):
        for i in range(nl):
            for n in ("norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias"):
                norms.append(sd[f"{pre}.layers.{i}.{n}"].contiguous())
    nl = lib.imcui_hip_loftr_num_layers()
    assert len(ws) == nl and len(norms) == lib.imcui_hip_loftr_num_norms(), (len(ws), nl)
    N, K = C.c_int(), C.c_int()
    w_np, b_np = [], []
    for i, (w, b) in enumerate(zip(ws, bs)):
        lib.imcui_hip_loftr_layer_shape(i, C.byref(N), C.byref(K))
        if tuple(w.shape) != (N.value, K.value):
            raise ImcuiHipError(f"LoFTR layer {i}: expected {(N.value, K.value)}, got {tuple(w.shape)}")
        w_np.append(_as_f32_host(w))
        b_np.append(None if b is None else _as_f32_host(b))
    n_np = [_as_f32_host(n) for n in norms]
    packed = np.zeros(lib.imcui_hip_loftr_packed_floats(), dtype=np.float32)
    wp = (C.c_void_p * nl)(*[a.ctypes.data for a in w_np])
    bp = (C.c_void_p * nl)(*[(0 if a is None else a.ctypes.data) for a in b_np])
    npp = (C.c_void_p * len(n_np))(*[a.ctypes.data for a in n_np])
    c1w, c1b = np.ascontiguousarray(conv1_w, dtype=np.float32), np.ascontiguousarray(conv1_b, dtype=np.float32)
    rc = lib.imcui_hip_loftr_pack_weights(c1w.ctypes.data, c1b.ctypes.data, wp, bp, npp, packed.ctypes.data)
    if rc != 0:
        raise ImcuiHipError(f"imcui_hip_loftr_pack_weights failed ({rc})")
    return torch.from_numpy(packed)


class _DenseMatcherHIP:
    """What LoFTR and EfficientLoFTR share: the input checks, the fixed-capacity outputs and `debug_buffer`, which reads intermediate maps
    out of the last forward's workspace (`last_ws`, `last_dims`)."""

    _debug_offset = ""  # the library's imcui_hip_*_debug_offset of the network

    def __init__(self):
        self._ws = _Workspace()
        self.last_ws = None

    def _inputs(self, name: str, image0: torch.Tensor, image1: torch.Tensor):
        """-> (handle, image0, image1, dims (B, H0, W0, H1, W1), outputs in the order of the ABI's output pointers)."""
        dev = image0.device
        hd = get_handle(dev)
        image0, image1 = image0.contiguous().float(), image1.contiguous().float()
        B, Cc, H0, W0 = image0.shape
        B1, C1, H1, W1 = image1.shape
        if Cc != 1 or C1 != 1 or B1 != B:
            raise ImcuiHipError(f"{name} expects two batches of 1-channel images of equal batch size")
        cap = B * (H0 // 8) * (W0 // 8)
        out = {
            "keypoints0": torch.empty((cap, 2), dtype=torch.float32, device=dev), "keypoints1": torch.empty((cap, 2), dtype=torch.float32, device=dev),
            "confidence": torch.empty((cap,), dtype=torch.float32, device=dev), "batch_indexes": torch.empty((cap,), dtype=torch.int32, device=dev),
            "num_matches": torch.zeros((1,), dtype=torch.int32, device=dev),
        }  # fmt: skip
        return hd, image0, image1, (B, H0, W0, H1, W1), out

    def debug_buffer(self, which: int, shape) -> torch.Tensor:
        """Workspace buffer `which` of the last forward (`_debug_offset`) viewed as float32 `shape`."""
        off = getattr(load_library(), self._debug_offset)(which, *self.last_dims)
        n = int(np.prod(shape))
        return self.last_ws[off : off + 4 * n].view(torch.float32).view(*shape)


class LoFTRHIP(_DenseMatcherHIP):
    _debug_offset = "imcui_hip_loftr_debug_offset"

    def forward(self, packed, image0, image1, match_threshold, temp_bug_fix=False):
        """kornia LoFTR.forward on image0 [B,1,H0,W0] / image1 [B,1,H1,W1] (sizes may differ between the two sides);
        fixed-capacity outputs + device match count.

        With the routing switch loftr_fine_sparse = 1 (the default) the call reads the coarse match count back to the host -- one
        synchronisation -- to choose between the dense last FPN stage and the 5x5 windows of the matches (`last_fine_mode`).  On a stream
        that is being captured into a HIP graph it takes the dense path and does not synchronise; loftr_fine_sparse = 0 never does."""
        hd, image0, image1, dims, out = self._inputs("LoFTR", image0, image1)
        with self._ws.use(hd.lib.imcui_hip_loftr_workspace_bytes(*dims), image0.device) as ws:
            self.last_ws, self.last_dims = ws, dims
            hd.launch(hd.lib.imcui_hip_loftr_forward, _ptr(packed), _ptr(image0), _ptr(image1), *dims, float(match_threshold), int(bool(temp_bug_fix)),
                      *map(_ptr, out.values()), _ptr(ws), ws.numel())  # fmt: skip
        return out

    @staticmethod
    def last_fine_mode(dev) -> tuple:
        """(mode, matches) of the last forward on this device's handle (imcui_hip_loftr_last_fine_mode): mode 0 = the last FPN stage as dense
        maps, 1 = on the 5x5 windows of the matches; matches = the count read back for that decision (-1: none)."""
        hd = get_handle(dev)
        m = C.c_int(-1)
        return int(hd.lib.imcui_hip_loftr_last_fine_mode(hd.h, C.byref(m))), m.value


# ------------------------------------------------------------------ EfficientLoFTR
def _repvgg_reparam(sd: dict, p: str, eps: float = 1e-5):
    """One RepVGG block (3x3 + BN, 1x1 + BN, optional identity BN) -> a single 3x3 convolution (w, b): the
    `reparameter()` step of the reference wrapper (eloftr.py:61), done in float64."""
    def branch(wk, bn):
        w = sd[wk].double()
        g = sd[bn + ".weight"].double() / torch.sqrt(sd[bn + ".running_var"].double() + eps)
        return w * g.view(-1, 1, 1, 1), sd[bn + ".bias"].double() - sd[bn + ".running_mean"].double() * g

    w3, b3 = branch(p + ".conv1.conv.weight", p + ".conv1.norm")
    w1, b1 = branch(p + ".conv2.conv.weight", p + ".conv2.norm")
    w = w3.clone()
    w[:, :, 1:2, 1:2] += w1
    b = b3 + b1
    if p + ".identity.weight" in sd:
        c = w.shape[0]
        g = sd[p + ".identity.weight"].double() / torch.sqrt(sd[p + ".identity.running_var"].double() + eps)
        w[torch.arange(c), torch.arange(c), 1, 1] += g
        b = b + sd[p + ".identity.bias"].double() - sd[p + ".identity.running_mean"].double() * g
    return w.float(), b.float()


def pack_eloftr(state_dict: dict) -> torch.Tensor:
    """EfficientLoFTR state dict (names of `transformers.EfficientLoFTRForKeypointMatching`) -> packed float32 buffer
    (host): RepVGG re-parameterisation, BatchNorm folding, GEMM layouts."""
    lib = load_library()
    sd = {k: v.detach().float().cpu() for k, v in state_dict.items() if isinstance(v, torch.Tensor)}
    bb = "efficientloftr.backbone.stages."
    w0, b0 = _repvgg_reparam(sd, bb + "0.blocks.0")
    conv0_w = np.ascontiguousarray(w0[:, 0].reshape(64, 9).t().numpy(), dtype=np.float32)  # [tap][cout]
    conv0_b = np.ascontiguousarray(b0.numpy(), dtype=np.float32)
    ws, bs = [], []
    for s, nb in ((1, 2), (2, 4), (3, 14)):
        for b in range(nb):
            w, bias = _repvgg_reparam(sd, f"{bb}{s}.blocks.{b}")
            wg, bg = _conv_gemm_layout(w, bias, w.shape[0], w.shape[1])
            ws.append(wg)
            bs.append(bg)
    tr = "efficientloftr.local_feature_transformer.layers."
    dws, norms = [], []
    for layer in range(4):
        for kind in ("self_attention", "cross_attention"):
            p = f"{tr}{layer}.{kind}."
            for n in ("attention.q_proj", "attention.k_proj", "attention.v_proj", "attention.o_proj", "mlp.fc1", "mlp.fc2"):
                ws.append(sd[p + n + ".weight"].contiguous())
                bs.append(None)
            dws.append(sd[p + "aggregation.q_aggregation.weight"].reshape(256, 16).contiguous())
            norms += [sd[p + "aggregation.norm.weight"], sd[p + "aggregation.norm.bias"], sd[p + "mlp.layer_norm.weight"], sd[p + "mlp.layer_norm.bias"]]
    rf = "refinement_layer."
    w = sd[rf + "out_conv.weight"] / 16.0  # coarse features enter the fusion divided by sqrt(256)
    wg, bg = _conv_gemm_layout(w, torch.zeros(w.shape[0]), w.shape[0], w.shape[1])
    ws.append(wg)
    bs.append(bg)
    for i in range(2):
        p = f"{rf}out_conv_layers.{i}."
        for wk, bn in ((p + "out_conv1", None), (p + "out_conv2", p + "batch_norm"), (p + "out_conv3", None)):
            w, bias = _fold_bn(sd[wk + ".weight"], sd, bn)
            wg, bg = _conv_gemm_layout(w, bias, w.shape[0], w.shape[1])
            ws.append(wg)
            bs.append(bg)
    nl = lib.imcui_hip_eloftr_num_layers()
    assert len(ws) == nl, (len(ws), nl)
    N, K = C.c_int(), C.c_int()
    w_np, b_np = [], []
    for i, (w, b) in enumerate(zip(ws, bs)):
        lib.imcui_hip_eloftr_layer_shape(i, C.byref(N), C.byref(K))
        if tuple(w.shape) != (N.value, K.value):
            raise ImcuiHipError(f"EfficientLoFTR layer {i}: expected {(N.value, K.value)}, got {tuple(w.shape)}")
        w_np.append(_as_f32_host(w))
        b_np.append(None if b is None else _as_f32_host(b))
    d_np = [_as_f32_host(d) for d in dws]
    n_np = [_as_f32_host(n) for n in norms]
    inv_freq = _as_f32_host(1.0 / (10000.0 ** (torch.arange(0, 128, 2, dtype=torch.float32) / 128)))  # the port's rope init, float32
    packed = np.zeros(lib.imcui_hip_eloftr_packed_floats(), dtype=np.float32)
    wp = (C.c_void_p * nl)(*[a.ctypes.data for a in w_np])
    bp = (C.c_void_p * nl)(*[(0 if a is None else a.ctypes.data) for a in b_np])
    dp = (C.c_void_p * 8)(*[a.ctypes.data for a in d_np])
    npp = (C.c_void_p * len(n_np))(*[a.ctypes.data for a in n_np])
    rc = lib.imcui_hip_eloftr_pack_weights(conv0_w.ctypes.data, conv0_b.ctypes.data, wp, bp, dp, npp, inv_freq.ctypes.data, packed.ctypes.data)
    if rc != 0:
        raise ImcuiHipError(f"imcui_hip_eloftr_pack_weights failed ({rc})")
    return torch.from_numpy(packed)


class ELoFTRHIP(_DenseMatcherHIP):
    _debug_offset = "imcui_hip_eloftr_debug_offset"

    def forward(self, packed, image0, image1, match_threshold, debug_windows=False, arith=0):
        """Upstream EfficientLoFTR forward on image0 [B,1,H0,W0] / image1 [B,1,H1,W1] (multiples of 32; the two sizes may
        differ); fixed-capacity outputs + device match count.  arith 1 = the wrapper's precision "fp16" / "mp" (one f16
        product per element pair in the convolutions)."""
        hd, image0, image1, dims, out = self._inputs("EfficientLoFTR", image0, image1)
        with self._ws.use(hd.lib.imcui_hip_eloftr_workspace_bytes(*dims, int(bool(debug_windows))), image0.device) as ws:
            self.last_ws, self.last_dims = ws, dims
            hd.launch(hd.lib.imcui_hip_eloftr_forward_ex, _ptr(packed), _ptr(image0), _ptr(image1), *dims, float(match_threshold), int(arith),
                      *map(_ptr, out.values()), int(bool(debug_windows)), _ptr(ws), ws.numel())  # fmt: skip
        return out


DUST3R_CFG = {"enc_dim": 1024, "enc_depth": 24, "dec_dim": 768, "dec_depth": 12, "desc_dim": 0}  # DUSt3R_ViTLarge_BaseDecoder_512_dpt


def _dust3r_c5(cfg: dict) -> tuple:
    return (cfg["enc_dim"], cfg["enc_depth"], cfg["dec_dim"], cfg["dec_depth"], cfg.get("desc_dim", 0))


def dust3r_cfg_of(state_dict: dict) -> dict:
    """Architecture of an `AsymmetricCroCo3DStereo` state dict (dims from the tensors, depths from the block indices)."""
    def depth(prefix):
        return 1 + max(int(k[len(prefix) :].split(".")[0]) for k in state_dict if k.startswith(prefix))

    return {
        "enc_dim": state_dict["patch_embed.proj.weight"].shape[0],
        "enc_depth": depth("enc_blocks."),
        "dec_dim": state_dict["decoder_embed.weight"].shape[0],
        "dec_depth": depth("dec_blocks."),
        # MASt3R: head_local_features.fc2 emits (desc_dim + 1) x 16 x 16 values per token
        "desc_dim": (state_dict["downstream_head1.head_local_features.fc2.weight"].shape[0] // 256 - 1) if "downstream_head1.head_local_features.fc2.weight" in state_dict else 0,
    }


def _fold_layernorm(w: torch.Tensor, b, gamma: torch.Tensor, beta: torch.Tensor):
    """(W, b) of a linear layer that reads LayerNorm(x; gamma, beta) -> (W * gamma, b + W beta): the layer then reads the plain
    normalisation of x.  float64 for the bias sum, one f32 rounding per weight."""
    w64 = w.double()
    b64 = (b.double() if b is not None else torch.zeros(w.shape[0], dtype=torch.float64)) + w64 @ beta.double()
    return (w64 * gamma.double()[None, :]).float(), b64.float()


def dust3r_matrices(state_dict: dict):
    """The matrices [N, K], biases and f32 vectors of a DUSt3R / MASt3R state dict in the order of the C layer table (what
    `pack_dust3r` hands to imcui_hip_dust3r_pack_weights) -> (cfg, matrices, biases, vectors).

    The affine part of every LayerNorm whose ONLY consumer is a linear layer is folded into that layer (round 3):
    `LN(x) W^T + b = xhat (W * gamma)^T + (b + W beta)` with `xhat = (x - mean) / sqrt(var + eps)`, so the device normalises without
    gamma / beta -- one pass serves `norm1` and the other side's `norm_y` of a decoder block (same input, different affine parts) and
    both decoder sides at once.  Folded: encoder norm1 -> attn.qkv, norm2 -> mlp.fc1; decoder norm1 -> attn.qkv, norm2 ->
    cross_attn.projq, norm_y -> cross_attn.projk / projv, norm3 -> mlp.fc1.  enc_norm and dec_norm feed the DPT heads as they are and stay
    LayerNorms.  The folded vectors are still handed over (layout unchanged); the device ignores them."""
    sd = {k: v.detach().float().cpu() for k, v in state_dict.items() if isinstance(v, torch.Tensor)}
    cfg = dust3r_cfg_of(sd)
    ws, bs, vecs = [], [], []

    def lin(name, ln=None):
        w = sd[name + ".weight"].reshape(sd[name + ".weight"].shape[0], -1)
        b = sd.get(name + ".bias")
        if ln is not None:
            w, b = _fold_layernorm(w, b, sd[ln + ".weight"], sd[ln + ".bias"])
        ws.append(w.contiguous())
        bs.append(b)

    def conv(name):  # OIHW -> [Cout][tap][Cin]
        w = sd[name + ".weight"]
        ws.append(w.permute(0, 2, 3, 1).reshape(w.shape[0], -1).contiguous())
        bs.append(sd.get(name + ".bias"))

    def deconv(name):  # [Cin][Cout][s][s] -> [(dy, dx, cout)][cin], bias tiled over (dy, dx)
        w = sd[name + ".weight"]
        s = w.shape[2]
        ws.append(w.permute(2, 3, 1, 0).reshape(s * s * w.shape[1], w.shape[0]).contiguous())
        bs.append(sd[name + ".bias"].repeat(s * s).contiguous())

    def norm(name):
        vecs.extend([sd[name + ".weight"], sd[name + ".bias"]])

    lin("patch_embed.proj")
    for i in range(cfg["enc_depth"]):
        p = f"enc_blocks.{i}."
        lin(p + "attn.qkv", p + "norm1")
        lin(p + "attn.proj")
        lin(p + "mlp.fc1", p + "norm2")
        lin(p + "mlp.fc2")
        norm(p + "norm1")
        norm(p + "norm2")
    norm("enc_norm")
    lin("decoder_embed")
    for blocks in ("dec_blocks", "dec_blocks2"):
        for i in range(cfg["dec_depth"]):
            p = f"{blocks}.{i}."
            lin(p + "attn.qkv", p + "norm1")
            lin(p + "attn.proj")
            lin(p + "cross_attn.projq", p + "norm2")
            # keys / values are projected from the OTHER stream's tokens, normalised by THIS block's norm_y
            wkv, bkv = _fold_layernorm(torch.cat((sd[p + "cross_attn.projk.weight"], sd[p + "cross_attn.projv.weight"]), 0),
                                       torch.cat((sd[p + "cross_attn.projk.bias"], sd[p + "cross_attn.projv.bias"]), 0),
                                       sd[p + "norm_y.weight"], sd[p + "norm_y.bias"])  # fmt: skip
            ws.append(wkv.contiguous())
            bs.append(bkv.contiguous())
            lin(p + "cross_attn.proj")
            lin(p + "mlp.fc1", p + "norm3")
            lin(p + "mlp.fc2")
            for n in ("norm1", "norm2", "norm_y", "norm3"):
                norm(p + n)
    norm("dec_norm")
    for hd in (1, 2):
        p = f"downstream_head{hd}.dpt."
        lin(p + "act_postprocess.0.0")
        deconv(p + "act_postprocess.0.1")
        lin(p + "act_postprocess.1.0")
        deconv(p + "act_postprocess.1.1")
        lin(p + "act_postprocess.2.0")
        lin(p + "act_postprocess.3.0")
        conv(p + "act_postprocess.3.1")
        for k in range(4):
            conv(f"{p}scratch.layer_rn.{k}")
        for r in (4, 3, 2, 1):
            for u in (1, 2):
                conv(f"{p}scratch.refinenet{r}.resConfUnit{u}.conv1")
                conv(f"{p}scratch.refinenet{r}.resConfUnit{u}.conv2")
            lin(f"{p}scratch.refinenet{r}.out_conv")
        conv(p + "head.0")
        conv(p + "head.2")
        if cfg["desc_dim"] > 0:
            lin(f"downstream_head{hd}.head_local_features.fc1")
            lin(f"downstream_head{hd}.head_local_features.fc2")
    for hd in (1, 2):
        p = f"downstream_head{hd}.dpt.head.4"
        vecs.extend([sd[p + ".weight"].reshape(4, 128).contiguous(), sd[p + ".bias"]])
    vecs.append(1.0 / (100.0 ** (torch.arange(0, 32, 2, dtype=torch.float32) / 32)))  # RoPE2D(freq=100), D = 32 per axis
    return cfg, ws, bs, vecs


def pack_dust3r(state_dict: dict) -> tuple[torch.Tensor, dict]:
    """`AsymmetricCroCo3DStereo` state dict (head_type 'dpt', upstream names; imcui/hloc/matchers/duster.py:37) -> (packed
    float32 host buffer, cfg).  Layer order and layouts: include/imcui_hip.h, the DUSt3R section."""
    lib = load_library()
    cfg, ws, bs, vecs = dust3r_matrices(state_dict)
    c4 = _dust3r_c5(cfg)
    nl = lib.imcui_hip_dust3r_num_layers(*c4)
    if nl == 0:
        raise ImcuiHipError(f"DUSt3R configuration {cfg} is not supported (dims multiples of 64 up to 1024, dec_depth a multiple of 4)")
    nv = lib.imcui_hip_dust3r_num_vectors(*c4)
    assert len(ws) == nl and len(vecs) == nv, (len(ws), nl, len(vecs), nv)
    N, K = C.c_int(), C.c_int()
    w_np, b_np, v_np = [], [], []
    for i, (w, b) in enumerate(zip(ws, bs)):
        lib.imcui_hip_dust3r_layer_shape(*c4, i, C.byref(N), C.byref(K))
        if tuple(w.shape) != (N.value, K.value):
            raise ImcuiHipError(f"DUSt3R layer {i}: expected {(N.value, K.value)}, got {tuple(w.shape)}")
        w_np.append(_as_f32_host(w))
        b_np.append(None if b is None else _as_f32_host(b))
    for i, v in enumerate(vecs):
        if v.numel() != lib.imcui_hip_dust3r_vector_len(*c4, i):
            raise ImcuiHipError(f"DUSt3R vector {i}: expected {lib.imcui_hip_dust3r_vector_len(*c4, i)} values, got {v.numel()}")
        v_np.append(_as_f32_host(v))
    packed = np.zeros(lib.imcui_hip_dust3r_packed_floats(*c4), dtype=np.float32)
    wp = (C.c_void_p * nl)(*[a.ctypes.data for a in w_np])
    bp = (C.c_void_p * nl)(*[(0 if a is None else a.ctypes.data) for a in b_np])
    vp = (C.c_void_p * nv)(*[a.ctypes.data for a in v_np])
    rc = lib.imcui_hip_dust3r_pack_weights(*c4, wp, bp, vp, packed.ctypes.data)
    if rc != 0:
        raise ImcuiHipError(f"imcui_hip_dust3r_pack_weights failed ({rc})")
    return torch.from_numpy(packed), cfg


def check_dust3r_packed(packed: torch.Tensor, cfg: dict) -> None:
    """Raise unless `packed` is a buffer THIS library's packer wrote for `cfg` (size and format trailer; include/imcui_hip.h, the DUSt3R
    section).  Called once when a module is built from conf["packed"] -- the documented way to skip the ~20 s of packing -- so that a blob
    cached from an older layout is refused instead of running with its LayerNorm affine parts dropped."""
    lib = load_library()
    c4 = _dust3r_c5(cfg)
    want = lib.imcui_hip_dust3r_packed_floats(*c4)
    if packed.dtype != torch.float32 or packed.numel() != want:
        raise ImcuiHipError(f"DUSt3R packed buffer: {packed.numel()} {packed.dtype} values, format {lib.imcui_hip_dust3r_format_version()} of this library needs "
                            f"{want} float32 -- a blob of another layout / configuration; pack the state dict again (backend.pack_dust3r)")
    if packed.device.type == "cpu":
        rc = lib.imcui_hip_dust3r_check_packed(*c4, packed.contiguous().data_ptr(), want)
    else:  # device-resident: bring the 64-word trailer (the last words of the buffer) to the host and compare it here
        tail = packed.reshape(-1)[-64:].detach().cpu().contiguous().view(torch.int32)[:9].tolist()
        fmt = lib.imcui_hip_dust3r_format_version()
        expect = [0x494D4455, fmt, want & 0xFFFFFFFF, want >> 32, *c4]
        rc = 0 if [v & 0xFFFFFFFF for v in tail] == [v & 0xFFFFFFFF for v in expect] else -1
    if rc != 0:
        raise ImcuiHipError(f"DUSt3R packed buffer: no format-{lib.imcui_hip_dust3r_format_version()} trailer for configuration {cfg} -- not written by this library's "
                            "imcui_hip_dust3r_pack_weights; pack the state dict again (backend.pack_dust3r)")


class DUSt3RHIP:
    def __init__(self):
        self._ws = _Workspace()
        self.last_dump = None

    @staticmethod
    def _check_inputs(hd: Handle, channels, pairs, NI: int) -> torch.Tensor:
        """The arithmetic mode, 3-channel images and a pair table inside [0, NI) -> the pair table as int32 [P,2]."""
        if hd.lib.imcui_hip_get_precision(hd.h) != 1:  # imcui_hip_dust3r_forward exists in the 3 x f16 split arithmetic only
            raise ImcuiHipError("DUSt3R / MASt3R run in the library's default arithmetic (imcui_hip_set_precision(h, 1)): the exact-f32 matrix "
                                "mode has no ViT kernels (for an exact-f32 nearest-neighbour search set conf['matcher_arithmetic'] = 'fp32')")
        if any(c != 3 for c in channels):
            raise ImcuiHipError("DUSt3R expects 3-channel images")
        pairs = torch.as_tensor(pairs, dtype=torch.int32).reshape(-1, 2)
        if int(pairs.min()) < 0 or int(pairs.max()) >= NI:
            raise ImcuiHipError(f"DUSt3R pair table refers to images outside [0, {NI})")
        return pairs

    def forward(self, packed, cfg, images, pairs, dump=False, arith=0):
        """images [NI,3,H,W] in [0,1] (H, W multiples of 16), pairs [P,2] int (view-1 image, view-2 image) ->
        {"pts3d": [2,P,H,W,3], "conf": [2,P,H,W]} (view 1 in its own frame, view 2 in view 1's frame); a MASt3R network
        (cfg["desc_dim"] > 0) also returns "desc" [2,P,H,W,desc_dim] and "desc_conf" [2,P,H,W].
        arith: 0 = 3 x f16 split products (fp32-grade), 1 = one f16 product per element pair (bf16-class)."""
        dev = images.device
        hd = get_handle(dev)
        lib = hd.lib
        images = images.contiguous().float()
        NI, Cc, H, W = images.shape
        pairs = self._check_inputs(hd, [Cc], pairs, NI).to(dev).contiguous()
        P = pairs.shape[0]
        c4 = _dust3r_c5(cfg)
        dd = c4[4]
        pts = torch.empty((2, P, H, W, 3), dtype=torch.float32, device=dev)
        conf = torch.empty((2, P, H, W), dtype=torch.float32, device=dev)
        desc = torch.empty((2, P, H, W, dd), dtype=torch.float32, device=dev) if dd else None
        dconf = torch.empty((2, P, H, W), dtype=torch.float32, device=dev) if dd else None
        nd = lib.imcui_hip_dust3r_dump_floats(*c4, NI, P, H, W) if dump else 0
        dbuf = torch.zeros((nd,), dtype=torch.float32, device=dev) if dump else None
        nbytes = lib.imcui_hip_dust3r_workspace_bytes(*c4, NI, P, H, W)
        if nbytes == 0:
            raise ImcuiHipError(f"DUSt3R: unsupported sizes ({NI} images of {W}x{H}, {P} pairs; multiples of 16)")
        with self._ws.use(nbytes, dev) as ws:
            hd.launch(lib.imcui_hip_dust3r_forward, *c4, _ptr(packed), packed.numel(), _ptr(images), NI, H, W, _ptr(pairs), P, int(arith), _ptr(pts), _ptr(conf),
                      _ptr(desc), _ptr(dconf), _ptr(dbuf), nd, _ptr(ws), ws.numel())  # fmt: skip
        self.last_dump = dbuf
        out = {"pts3d": pts, "conf": conf}
        if dd:
            out.update(desc=desc, desc_conf=dconf)
        return out

    def forward_sizes(self, packed, cfg, images, pairs, dump=False, arith=0):
        """The same network on images of several sizes (imcui_hip_dust3r_forward_sizes): `images` = list of [3,H_i,W_i] (or
        [1,3,H_i,W_i]) tensors in [0,1], every size a multiple of 16, at most 4 distinct sizes; pairs [P,2] ->
        {"pts3d": [view][pair] -> [H,W,3], "conf": [view][pair] -> [H,W]} (+ "desc" / "desc_conf" for a MASt3R network) as nested
        lists of views into ONE ragged device buffer per output: the map of (view v, pair p) has the size of image pairs[p][v]."""
        imgs = [im.reshape(im.shape[-3:]).contiguous().float() for im in images]
        dev = imgs[0].device
        hd = get_handle(dev)
        lib = hd.lib
        NI = len(imgs)
        ptab = self._check_inputs(hd, [im.shape[0] for im in imgs], pairs, NI).cpu().contiguous()
        sizes = [(int(im.shape[1]), int(im.shape[2])) for im in imgs]
        P = ptab.shape[0]
        flat = torch.cat([im.reshape(-1) for im in imgs])
        pairs_dev = ptab.to(dev)
        c4 = _dust3r_c5(cfg)
        dd = c4[4]
        sz = (C.c_int * (2 * NI))(*[v for hw in sizes for v in hw])
        ph = (C.c_int * (2 * P))(*[int(v) for v in ptab.reshape(-1)])
        offs = (C.c_size_t * (2 * P + 1))()
        total = sum(sizes[int(ptab[p, v])][0] * sizes[int(ptab[p, v])][1] for v in range(2) for p in range(P))
        pts = torch.empty((total, 3), dtype=torch.float32, device=dev)
        conf = torch.empty((total,), dtype=torch.float32, device=dev)
        desc = torch.empty((total, dd), dtype=torch.float32, device=dev) if dd else None
        dconf = torch.empty((total,), dtype=torch.float32, device=dev) if dd else None
        # (images that all share one size take the one-size path inside the library, which also dumps the DPT head tensors)
        one_size = len(set(sizes)) == 1
        nd = (lib.imcui_hip_dust3r_dump_floats(*c4, NI, P, *sizes[0]) if one_size else lib.imcui_hip_dust3r_token_dump_floats(*c4, NI, sz, P)) if dump else 0
        dbuf = torch.zeros((nd,), dtype=torch.float32, device=dev) if dump else None
        nbytes = lib.imcui_hip_dust3r_workspace_bytes_sizes(*c4, NI, sz, P)
        if nbytes == 0:
            raise ImcuiHipError(f"DUSt3R: unsupported sizes {sizes} (multiples of 16, 32 .. 4096)")
        with self._ws.use(nbytes, dev) as ws:
            hd.launch(lib.imcui_hip_dust3r_forward_sizes, *c4, _ptr(packed), packed.numel(), _ptr(flat), NI, sz, ph, _ptr(pairs_dev), P, int(arith), _ptr(pts),
                      _ptr(conf), _ptr(desc), _ptr(dconf), offs, _ptr(dbuf), nd, _ptr(ws), ws.numel())  # fmt: skip
        assert offs[2 * P] == total
        self.last_dump = dbuf

        def maps(buf, tail):
            out = []
            for v in range(2):
                row = []
                for p in range(P):
                    Hh, Ww = sizes[int(ptab[p, v])]
                    o = offs[v * P + p]
                    row.append(buf[o : o + Hh * Ww].reshape((Hh, Ww) + tail))
                out.append(row)
            return out

        out = {"pts3d": maps(pts, (3,)), "conf": maps(conf, ())}
        if dd:
            out.update(desc=maps(desc, (dd,)), desc_conf=maps(dconf, ()))
        return out


def conv_gemm_f32(x_nhwc, w_oihw, bias, resid=None, stride=1, act=0):
    """Building block: NHWC conv through the implicit-im2col GEMM (k in {1,3}, Cin % 32 == 0)."""
    hd = get_handle(x_nhwc.device)
    B, H, W, Cin = x_nhwc.shape
    Cout, _, ks, _ = w_oihw.shape
    wg, bg = _conv_gemm_layout(w_oihw.float().cpu(), bias.float().cpu(), Cout, Cin)
    pad = ks // 2
    ho, wo = (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1
    out = torch.empty((B, ho, wo, Cout), dtype=torch.float32, device=x_nhwc.device)
    wd, bd = wg.to(x_nhwc.device), bg.to(x_nhwc.device)
    x_nhwc = x_nhwc.contiguous().float()
    if resid is not None:
        resid = resid.contiguous().float()
    hd.launch(hd.lib.imcui_hip_conv_gemm_f32, _ptr(x_nhwc), _ptr(wd), _ptr(bd), _ptr(resid), _ptr(out), B, H, W, Cin, Cout, ks, stride, act)
    return out


# ------------------------------------------------------------------ LISRD
LISRD_DESC, LISRD_META, LISRD_CLUSTERS, LISRD_TILE, LISRD_HIDDEN = 128, 128, 8, 3, 256
LISRD_DM = LISRD_CLUSTERS * LISRD_META
LISRD_MIN_SIDE = 8 * LISRD_TILE
LISRD_KINDS = ("stem", "conv3x3", "heads", "conv1x1")


def lisrd_layers() -> list[dict]:
    """The launch list as the library's ONE table states it (csrc/lisrd.hip, LISRD_LAYERS)."""
    lib = load_library()
    out = []
    for i in range(lib.imcui_hip_lisrd_num_layers()):
        v = (C.c_int * 5)()
        name = lib.imcui_hip_lisrd_layer(i, v).decode()
        out.append({"name": name, "kind": LISRD_KINDS[v[0]], "cin": v[1], "cout": v[2], "pool": v[3], "in_off": v[4]})
    return out


def lisrd_tensor_names() -> list[str]:
    lib = load_library()
    return [lib.imcui_hip_lisrd_tensor_name(i).decode() for i in range(lib.imcui_hip_lisrd_num_tensors())]


def lisrd_tensor_shapes() -> dict:
    """Shape of every tensor the packer takes, as the library states it (imcui_hip_lisrd_tensor_shape)."""
    lib = load_library()
    shapes = {}
    for i, name in enumerate(lisrd_tensor_names()):
        d = (C.c_int * 4)()
        shapes[name] = tuple(d[: lib.imcui_hip_lisrd_tensor_shape(i, d)])
    return shapes


def lisrd_variances() -> tuple:
    """The four variances in the order the wrapper's dictionaries iterate in, as the library states them."""
    lib = load_library()
    return tuple(lib.imcui_hip_lisrd_variance(v).decode() for v in range(4))


def pack_lisrd(state_dict: dict) -> torch.Tensor:
    """LISRD state dict (the keys of tests/lisrd_reference.py, which restate upstream's attribute names) -> packed float32 buffer (host).
    The BatchNorms (eval) become the affine y = x a + b behind the ReLU.  Strict: `num_batches_tracked` counters are ignored, every other
    key is consumed exactly once and every shape checked, so a checkpoint of another configuration than LISRD_CONFIG is refused by name."""
    lib = load_library()
    sd = {k: t for k, t in state_dict.items() if not k.endswith("num_batches_tracked")}
    return _pack_named("LISRD", "the LISRD_CONFIG", lisrd_tensor_names(), lisrd_tensor_shapes(), sd, lib.imcui_hip_lisrd_packed_floats(), lib.imcui_hip_lisrd_pack_weights)


def lisrd_check_args(image_shape) -> None:
    """Refusals raised before anything is launched."""
    if len(image_shape) != 4 or image_shape[1] != 3:
        raise ValueError(f"LISRD expects a 3-channel image [B,3,H,W], got shape {tuple(image_shape)}")
    if image_shape[2] < LISRD_MIN_SIDE or image_shape[3] < LISRD_MIN_SIDE:
        raise ValueError(f"LISRD needs images of at least {LISRD_MIN_SIDE} x {LISRD_MIN_SIDE} (a region of the 1/8-resolution map without cells), got {tuple(image_shape[2:])}")


class LisrdHIP:
    def __init__(self):
        self._ws = _Workspace()

    def describe(self, packed: torch.Tensor, image: torch.Tensor, keypoints: torch.Tensor, counts: torch.Tensor) -> dict:
        """image [B,3,H,W] in [0,1] on the GPU, keypoints [B,K,2] (x, y) in pixels, counts [B] int32 -> desc [B,K,4,128], meta [B,K,4,1024]
        (unit vectors, rows past the count zero), status [1] int32.  Never synchronises."""
        lisrd_check_args(tuple(image.shape))
        hd = get_handle(image.device)
        _same_device(packed, image)
        image, keypoints = image.contiguous().float(), keypoints.contiguous().float()
        counts = counts.to(image.device, torch.int32).contiguous()
        B, Cc, H, W = image.shape
        K = keypoints.shape[1]
        if tuple(keypoints.shape) != (B, K, 2) or counts.numel() != B or K < 1:
            raise ImcuiHipError(f"LISRD: keypoints {tuple(keypoints.shape)} / counts {tuple(counts.shape)} do not belong to {B} images")
        dev = image.device
        out = {"desc": torch.empty((B, K, 4, LISRD_DESC), dtype=torch.float32, device=dev), "meta": torch.empty((B, K, 4, LISRD_DM), dtype=torch.float32, device=dev),
               "status": torch.empty((1,), dtype=torch.int32, device=dev)}  # fmt: skip
        with self._ws.use(hd.lib.imcui_hip_lisrd_describe_workspace_bytes(B, H, W), dev) as ws:
            hd.launch(hd.lib.imcui_hip_lisrd_describe, _ptr(packed), _ptr(image), B, Cc, H, W, _ptr(keypoints), _ptr(counts), K, _ptr(out["desc"]), _ptr(out["meta"]),
                      _ptr(out["status"]), _ptr(ws), ws.numel())  # fmt: skip
        return out

    def dense(self, packed: torch.Tensor, image: torch.Tensor) -> dict:
        """Test entry: descriptors [4][B,Hc,Wc,128] and raw meta maps [4][B,Hc,Wc,128] (NHWC, un-normalised), meta_descriptors [B,4,3,3,1024]."""
        lisrd_check_args(tuple(image.shape))
        hd = get_handle(image.device)
        image = image.contiguous().float()
        B, Cc, H, W = image.shape
        dense = torch.empty((8, B, H // 8, W // 8, 128), dtype=torch.float32, device=image.device)
        vlad = torch.empty((B, 4, LISRD_TILE, LISRD_TILE, LISRD_DM), dtype=torch.float32, device=image.device)
        with self._ws.use(hd.lib.imcui_hip_lisrd_describe_workspace_bytes(B, H, W), image.device) as ws:
            hd.launch(hd.lib.imcui_hip_lisrd_dense, _ptr(packed), _ptr(image), B, Cc, H, W, _ptr(dense), _ptr(vlad), _ptr(ws), ws.numel())
        return {"descriptors": dense[:4], "meta_maps": dense[4:], "meta_descriptors": vlad}

    def layers_probe(self, packed: torch.Tensor, x: torch.Tensor, first: int, last: int) -> torch.Tensor:
        """Test entry: entries [first, last] of `lisrd_layers` through the forward's own launch list on x: the planar image [B,3,H,W] when
        first == 0, else an NHWC map -> the last entry's NHWC map."""
        hd = get_handle(x.device)
        x = x.contiguous().float()
        B, H, W = (x.shape[0], x.shape[2], x.shape[3]) if first == 0 else tuple(x.shape[:3])
        hh, ww = H, W
        layers = lisrd_layers()
        for L in layers[first : last + 1]:
            if L["pool"]:
                hh, ww = hh // 2, ww // 2
        out = torch.empty((B, hh, ww, layers[last]["cout"]), dtype=torch.float32, device=x.device)
        with self._ws.use(max(256, hd.lib.imcui_hip_lisrd_layers_workspace_bytes(first, last, B, H, W)), x.device) as ws:
            hd.launch(hd.lib.imcui_hip_lisrd_layers_probe, _ptr(packed), _ptr(x), first, last, B, H, W, _ptr(out), _ptr(ws), ws.numel())
        return out

    @staticmethod
    def affine_probe(x: torch.Tensor, a: torch.Tensor, b: torch.Tensor, pool: bool) -> torch.Tensor:
        """Test entry: y = x a + b on x [B,H,W,C] (NHWC), through AvgPool2d(2, 2) when `pool`."""
        hd = get_handle(x.device)
        x, a, b = x.contiguous().float(), a.contiguous().float(), b.contiguous().float()
        B, H, W, Cc = x.shape
        out = torch.empty((B, H // 2, W // 2, Cc) if pool else (B, H, W, Cc), dtype=torch.float32, device=x.device)
        hd.launch(hd.lib.imcui_hip_lisrd_affine_probe, _ptr(x), _ptr(a), _ptr(b), B, H, W, Cc, int(bool(pool)), _ptr(out))
        return out

    def vlad_probe(self, packed: torch.Tensor, v: int, fmap: torch.Tensor) -> torch.Tensor:
        """Test entry: regional NetVLAD with variance v's weights on fmap [B,hc,wc,128] -> [B,3,3,1024]."""
        hd = get_handle(fmap.device)
        fmap = fmap.contiguous().float()
        B, hc, wc, _ = fmap.shape
        out = torch.empty((B, LISRD_TILE, LISRD_TILE, LISRD_DM), dtype=torch.float32, device=fmap.device)
        with self._ws.use(max(256, hd.lib.imcui_hip_lisrd_vlad_workspace_bytes(B, hc, wc)), fmap.device) as ws:
            hd.launch(hd.lib.imcui_hip_lisrd_vlad_probe, _ptr(packed), int(v), _ptr(fmap), B, hc, wc, _ptr(out), _ptr(ws), ws.numel())
        return out

    @staticmethod
    def sample_probe(dmaps: torch.Tensor, vlad: torch.Tensor, image_size: tuple, keypoints: torch.Tensor, counts: torch.Tensor) -> dict:
        """Test entry: the sparse sampling of dmaps [4,B,hc,wc,128] and vlad [B,4,3,3,1024] at keypoints [B,K,2] (x, y) of H x W images."""
        hd = get_handle(dmaps.device)
        dmaps, vlad, keypoints = dmaps.contiguous().float(), vlad.contiguous().float(), keypoints.contiguous().float()
        counts = counts.to(dmaps.device, torch.int32).contiguous()
        _, B, hc, wc, _ = dmaps.shape
        K = keypoints.shape[1]
        out = {"desc": torch.empty((B, K, 4, LISRD_DESC), dtype=torch.float32, device=dmaps.device),
               "meta": torch.empty((B, K, 4, LISRD_DM), dtype=torch.float32, device=dmaps.device)}  # fmt: skip
        hd.launch(hd.lib.imcui_hip_lisrd_sample_probe, _ptr(dmaps), _ptr(vlad), B, hc, wc, int(image_size[0]), int(image_size[1]), _ptr(keypoints), _ptr(counts), K,
                  _ptr(out["desc"]), _ptr(out["meta"]))  # fmt: skip
        return out


# ------------------------------------------------------------------ mutual NN
_nn_ws = _Workspace()


def mutual_nn(desc0_nd: torch.Tensor, desc1_md: torch.Tensor, ratio_threshold=None, distance_threshold=None,
              do_mutual_check=True):  # fmt: skip
    """desc0 [B,N,D], desc1 [B,M,D] (row per descriptor) -> matches0 [B,N] int32, scores0 [B,N]."""
    dev = desc0_nd.device
    hd = get_handle(dev)
    lib = hd.lib
    desc0_nd, desc1_md = desc0_nd.contiguous().float(), desc1_md.contiguous().float()
    B, N, D = desc0_nd.shape
    M = desc1_md.shape[1]
    m0 = torch.empty((B, N), dtype=torch.int32, device=dev)
    s0 = torch.empty((B, N), dtype=torch.float32, device=dev)
    if D % 32:
        raise ImcuiHipError(f"descriptor dim {D} must be a multiple of 32")
    # (no similarity matrix for D = 64 / 128 / 256 or the split arithmetic)
    with _nn_ws.use(lib.imcui_hip_mutual_nn_workspace_bytes_d(hd.h, B, N, M, D), dev) as ws:
        hd.launch(lib.imcui_hip_mutual_nn, _ptr(desc0_nd), _ptr(desc1_md), B, N, M, D, float(ratio_threshold or 0.0),
                  float(distance_threshold or 0.0), int(bool(do_mutual_check)), _ptr(m0), _ptr(s0), _ptr(ws), ws.numel())  # fmt: skip
    return m0, s0


def mutual_nn_dn(desc0_dn: torch.Tensor, desc1_dm: torch.Tensor, ratio_threshold=None, distance_threshold=None, do_mutual_check=True):
    """`mutual_nn` on the layout `NearestNeighbor._forward` receives: desc0 [B,D,N], desc1 [B,D,M] (column per descriptor); the transpose
    runs on the device inside the call (imcui_hip_mutual_nn_dn) -> matches0 [B,N] int32, scores0 [B,N]."""
    dev = desc0_dn.device
    hd = get_handle(dev)
    lib = hd.lib
    desc0_dn, desc1_dm = desc0_dn.contiguous().float(), desc1_dm.contiguous().float()
    B, D, N = desc0_dn.shape
    M = desc1_dm.shape[2]
    m0 = torch.empty((B, N), dtype=torch.int32, device=dev)
    s0 = torch.empty((B, N), dtype=torch.float32, device=dev)
    if D % 32:
        raise ImcuiHipError(f"descriptor dim {D} must be a multiple of 32")
    with _nn_ws.use(lib.imcui_hip_mutual_nn_dn_workspace_bytes_for(hd.h, B, N, M, D), dev) as ws:
        hd.launch(lib.imcui_hip_mutual_nn_dn, _ptr(desc0_dn), _ptr(desc1_dm), B, N, M, D, float(ratio_threshold or 0.0), float(distance_threshold or 0.0),
                  int(bool(do_mutual_check)), _ptr(m0), _ptr(s0), _ptr(ws), ws.numel())  # fmt: skip
    return m0, s0


def lisrd_match(desc0: torch.Tensor, meta0: torch.Tensor, desc1: torch.Tensor, meta1: torch.Tensor, cnt0: torch.Tensor | None = None,
                cnt1: torch.Tensor | None = None, want_nn: bool = False) -> dict:
    """LISRD's meta-weighted mutual nearest neighbours and the confidence of the matched pairs (imcui_hip_lisrd_match): desc0 [B,N,4,128],
    meta0 [B,N,4,Dm], desc1 [B,M,4,128], meta1 [B,M,4,Dm]; cnt0 / cnt1 [B] int32 on the device = live key-points per image (None: all).
    Returns matches0 [B,N] int32 (-1 = none), best0 [B,N] (row-best similarity), mconf [B,N] (0 where unmatched) and, with want_nn, the
    row / column arg-maxima nn12 [B,N] / nn21 [B,M] and the column-best similarity best1 [B,M].  Never synchronises."""
    dev = desc0.device
    hd = get_handle(dev)
    lib = hd.lib
    desc0, meta0, desc1, meta1 = (t.contiguous().float() for t in (desc0, meta0, desc1, meta1))
    if desc0.dim() != 4 or meta0.dim() != 4 or desc1.dim() != 4 or meta1.dim() != 4:
        raise ImcuiHipError("lisrd_match: descriptors are [B,K,4,128] and meta descriptors [B,K,4,Dm]")
    B, N, V, D = desc0.shape
    M, Dm = desc1.shape[1], meta0.shape[3]
    if (V, D) != (4, 128) or tuple(desc1.shape) != (B, M, 4, 128) or tuple(meta0.shape) != (B, N, 4, Dm) or tuple(meta1.shape) != (B, M, 4, Dm):
        raise ImcuiHipError(f"lisrd_match: shapes {tuple(desc0.shape)}, {tuple(meta0.shape)}, {tuple(desc1.shape)}, {tuple(meta1.shape)} do not belong together")
    if min(B, N, M) < 1 or Dm % 128 or not 128 <= Dm <= 1024:
        raise ImcuiHipError(f"lisrd_match: B={B}, N={N}, M={M} must be positive and the meta width {Dm} a multiple of 128 up to 1024")
    for c in (cnt0, cnt1):
        if c is not None and (c.dtype != torch.int32 or c.device != dev or c.numel() != B or not c.is_contiguous()):
            raise ImcuiHipError("lisrd_match: counts are contiguous int32 [B] tensors on the descriptors' device")
    out = {"matches0": torch.empty((B, N), dtype=torch.int32, device=dev), "best0": torch.empty((B, N), dtype=torch.float32, device=dev),
           "mconf": torch.empty((B, N), dtype=torch.float32, device=dev)}  # fmt: skip
    if want_nn:
        out["nn12"] = torch.empty((B, N), dtype=torch.int32, device=dev)
        out["nn21"] = torch.empty((B, M), dtype=torch.int32, device=dev)
        out["best1"] = torch.empty((B, M), dtype=torch.float32, device=dev)
    with _nn_ws.use(lib.imcui_hip_lisrd_match_workspace_bytes(B, N, M, Dm), dev) as ws:
        hd.launch(lib.imcui_hip_lisrd_match, _ptr(desc0), _ptr(meta0), _ptr(cnt0), _ptr(desc1), _ptr(meta1), _ptr(cnt1), B, N, M, Dm, _ptr(out["matches0"]),
                  _ptr(out["best0"]), _ptr(out["mconf"]), _ptr(out.get("nn12")), _ptr(out.get("nn21")), _ptr(out.get("best1")), _ptr(ws), ws.numel())  # fmt: skip
    return out


def nn_argmax(queries: torch.Tensor, db: torch.Tensor, return_best: bool = False, split: bool = False):
    """queries [Q,D], db [N,D] (D in 16 / 24 / 32) -> int64 [Q]: the FIRST arg-max over n of <queries[q], db[n]> (what
    `cdistMatcher(dist="dot").query` of upstream's mast3r/fast_nn.py returns; imcui/hloc/matchers/mast3r.py:68-75).
    split=True: the 3 x f16 split arithmetic (4 x fewer matrix cycles, fp32-grade values; near-ties may resolve differently)."""
    dev = queries.device
    hd = get_handle(dev)
    lib = hd.lib
    queries, db = queries.contiguous().float(), db.contiguous().float()
    Q, D = queries.shape
    N = db.shape[0]
    idx = torch.empty((Q,), dtype=torch.int32, device=dev)
    best = torch.empty((Q,), dtype=torch.float32, device=dev) if return_best else None
    if Q == 0:
        return (idx.long(), best) if return_best else idx.long()
    fn_ws, fn = ((lib.imcui_hip_nn_argmax_split_workspace_bytes, lib.imcui_hip_nn_argmax_split_f32) if split else
                 (lib.imcui_hip_nn_argmax_workspace_bytes, lib.imcui_hip_nn_argmax_f32))
    with _nn_ws.use(fn_ws(Q, N), dev) as ws:
        hd.launch(fn, _ptr(queries), _ptr(db), Q, N, D, _ptr(idx), _ptr(best), _ptr(ws), ws.numel())
    return (idx.long(), best) if return_best else idx.long()


def dual_softmax(desc0: torch.Tensor, desc1: torch.Tensor, threshold: float = 0.2, inv_temperature: float = 20.0, normalize: bool = True):
    """desc0 [B,C,N], desc1 [B,C,M] (channels-first, as the plugin receives them) -> matches0 [B,N] int32, scores0 [B,N]."""
    dev = desc0.device
    hd = get_handle(dev)
    lib = hd.lib
    desc0, desc1 = desc0.contiguous().float(), desc1.contiguous().float()
    B, C, N = desc0.shape
    M = desc1.shape[2]
    m0 = torch.empty((B, N), dtype=torch.int32, device=dev)
    s0 = torch.empty((B, N), dtype=torch.float32, device=dev)
    with _nn_ws.use(lib.imcui_hip_dual_softmax_workspace_bytes(B, C, N, M), dev) as ws:
        hd.launch(lib.imcui_hip_dual_softmax, _ptr(desc0), _ptr(desc1), B, C, N, M, float(threshold), float(inv_temperature),
                  int(bool(normalize)), _ptr(m0), _ptr(s0), _ptr(ws), ws.numel())  # fmt: skip
    return m0, s0


# ------------------------------------------------------------------ arithmetic mode
def set_precision(device: torch.device, mode: int):
    """0 = exact f32 MFMA, 1 = 3 x f16 split MFMA (default; ~fp32 accuracy at ~5x the matrix rate)."""
    hd = get_handle(device)
    hd.call(hd.lib.imcui_hip_set_precision, int(mode))


def get_precision(device: torch.device) -> int:
    hd = get_handle(device)
    return hd.lib.imcui_hip_get_precision(hd.h)


def lib_version() -> int:
    """imcui_hip_version() of the loaded library (400 since round 4: packed-buffer formats are tied to it)."""
    return int(load_library().imcui_hip_version())


def set_option(device: torch.device, name: str, value: int) -> int:
    """A/B switch of the kernel routing (imcui_hip_set_option: "gemm_wreg", "wreg_pipe", "attn_variant", "attn_variant_self", "attn_variant_cross", "attn_mix_layers", "simred", "ffn_tile", "wreg_tile", "conv_tall", "conv_narrow", "attn_split", "loftr_fine_sparse"); returns
    the previous value.  The IMCUI_* environment variables of the same names are only read when the handle is created."""
    hd = get_handle(device)
    old = C.c_int(0)
    hd.call(hd.lib.imcui_hip_get_option, name.encode(), C.byref(old))
    hd.call(hd.lib.imcui_hip_set_option, name.encode(), int(value))
    return old.value


def get_option(device: torch.device, name: str) -> int:
    """Current value of a routing switch (imcui_hip_get_option)."""
    hd = get_handle(device)
    val = C.c_int(0)
    hd.call(hd.lib.imcui_hip_get_option, name.encode(), C.byref(val))
    return val.value


class option:
    """`with backend.option(dev, attn_variant=6): ...` -- set switches for a block of calls and restore them afterwards."""

    def __init__(self, device: torch.device, **kw):
        self.device, self.kw, self.old = device, kw, {}

    def __enter__(self):
        for k, v in self.kw.items():
            self.old[k] = set_option(self.device, k, v)
        return self

    def __exit__(self, *a):
        for k, v in self.old.items():
            set_option(self.device, k, v)


# ------------------------------------------------------------------ live kernel timing
KERNEL_CLASSES = {"attention": 0, "conv3x3": 1, "gemm": 2}


def profile_enable(device: torch.device, on: bool = True):
    hd = get_handle(device)
    hd.call(hd.lib.imcui_hip_profile_enable, int(on))


def profile_read(device: torch.device, kernel_class: str):
    """(total kernel ms, launches) of one class since the last read; HIP events on the launch stream."""
    hd = get_handle(device)
    tot, cnt = C.c_double(0.0), C.c_int(0)
    hd.call(hd.lib.imcui_hip_profile_read, KERNEL_CLASSES[kernel_class], C.byref(tot), C.byref(cnt))
    return tot.value, cnt.value


# ------------------------------------------------------------------ building blocks (tests)
def linear_f32(a: torch.Tensor, w: torch.Tensor, bias: torch.Tensor | None, relu: bool = False) -> torch.Tensor:
    hd = get_handle(a.device)
    a, w = a.contiguous().float(), w.contiguous().float()
    M, K = a.shape
    N = w.shape[0]
    c = torch.empty((M, N), dtype=torch.float32, device=a.device)
    hd.launch(hd.lib.imcui_hip_linear_f32, _ptr(a), _ptr(w), _ptr(bias), _ptr(c), M, N, K, int(relu))
    return c


def rgb_to_gray(rgb_u8: torch.Tensor) -> torch.Tensor:
    """Device-side `cv2.cvtColor(RGB2GRAY)` + `astype(float32) / 255` (extract_features.py:120-160) for decoded
    uint8 images [B,H,W,3] already on the device -> [B,1,H,W] float32 in [0,1]."""
    if rgb_u8.dtype != torch.uint8 or rgb_u8.dim() != 4 or rgb_u8.shape[-1] != 3:
        raise ImcuiHipError("rgb_to_gray expects uint8 [B,H,W,3]")
    hd = get_handle(rgb_u8.device)
    rgb_u8 = rgb_u8.contiguous()
    B, H, W, _ = rgb_u8.shape
    out = torch.empty((B, 1, H, W), dtype=torch.float32, device=rgb_u8.device)
    hd.launch(hd.lib.imcui_hip_rgb_to_gray_f32, _ptr(rgb_u8), _ptr(out), B, H, W)
    return out


_area_tables: dict = {}


def _area_table(ssize: int, dsize: int, device: torch.device):
    """OpenCV INTER_AREA decimation table ssize -> dsize as device tensors (start [dsize+1], index, weight); cached."""
    key = (ssize, dsize, str(device))
    if key not in _area_tables:
        lib = load_library()
        start = np.zeros(dsize + 1, dtype=np.int32)
        n = lib.imcui_hip_area_table(ssize, dsize, start.ctypes.data, None, None)
        if n <= 0:
            raise ImcuiHipError(f"area table {ssize} -> {dsize}: only shrinking resizes are supported")
        idx, wgt = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.float32)
        lib.imcui_hip_area_table(ssize, dsize, start.ctypes.data, idx.ctypes.data, wgt.ctypes.data)
        _area_tables[key] = tuple(torch.from_numpy(a).to(device) for a in (start, idx, wgt))
    return _area_tables[key]


def preprocess_area(img_u8: torch.Tensor, size) -> torch.Tensor:
    """Device-side `extract.preprocess` with a resize (extract_features.py:120-148): uint8 [B,H,W] / [B,H,W,1] gray or
    [B,H,W,3] RGB on the device -> gray (cv2 fixed point) -> float32 -> cv2.INTER_AREA to `size` = (w, h) -> / 255 ->
    float32 [B,1,h,w].  Shrinking resizes only."""
    if img_u8.dtype != torch.uint8 or img_u8.dim() not in (3, 4):
        raise ImcuiHipError("preprocess_area expects uint8 [B,H,W] or [B,H,W,C]")
    if img_u8.dim() == 3:
        img_u8 = img_u8[..., None]
    hd = get_handle(img_u8.device)
    img_u8 = img_u8.contiguous()
    B, H, W, Cc = img_u8.shape
    ow, oh = int(size[0]), int(size[1])
    out = torch.empty((B, 1, oh, ow), dtype=torch.float32, device=img_u8.device)
    tabs = [None] * 6
    if not (W % ow == 0 and H % oh == 0) and ow <= W and oh <= H:
        tabs = [*_area_table(W, ow, img_u8.device), *_area_table(H, oh, img_u8.device)]
    hd.launch(hd.lib.imcui_hip_preprocess_area_f32, _ptr(img_u8), B, H, W, Cc, *[_ptr(t) for t in tabs], _ptr(out), oh, ow)
    return out


def preprocess_area_rgb(img_u8: torch.Tensor, size) -> torch.Tensor:
    """The RGB branch of `extract.preprocess` (extract_features.py:80-99, `grayscale: False`): uint8 [B,H,W,3] on the device ->
    float32 -> cv2.INTER_AREA per channel to `size` = (w, h) -> / 255 -> float32 planar [B,3,h,w].  `size` equal to the input
    converts without resizing; shrinking resizes only."""
    if img_u8.dtype != torch.uint8 or img_u8.dim() != 4 or img_u8.shape[-1] != 3:
        raise ImcuiHipError("preprocess_area_rgb expects uint8 [B,H,W,3]")
    hd = get_handle(img_u8.device)
    img_u8 = img_u8.contiguous()
    B, H, W, _ = img_u8.shape
    ow, oh = int(size[0]), int(size[1])
    out = torch.empty((B, 3, oh, ow), dtype=torch.float32, device=img_u8.device)
    tabs = [None] * 6
    if not (W % ow == 0 and H % oh == 0) and ow <= W and oh <= H:
        tabs = [*_area_table(W, ow, img_u8.device), *_area_table(H, oh, img_u8.device)]
    hd.launch(hd.lib.imcui_hip_preprocess_area_rgb_f32, _ptr(img_u8), B, H, W, *[_ptr(t) for t in tabs], _ptr(out), oh, ow)
    return out


_linear_tables: dict = {}
_aa_tables: dict = {}


def linear_table_host(ssize: int, dsize: int, horizontal: bool):
    """cv2.INTER_LINEAR tap table (host numpy): (i0, i1, w1)."""
    lib = load_library()
    i0, i1, w1 = np.zeros(dsize, dtype=np.int32), np.zeros(dsize, dtype=np.int32), np.zeros(dsize, dtype=np.float32)
    if lib.imcui_hip_linear_table(ssize, dsize, int(horizontal), i0.ctypes.data, i1.ctypes.data, w1.ctypes.data) != 0:
        raise ImcuiHipError(f"linear table {ssize} -> {dsize}")
    return i0, i1, w1


def aa_table_host(in_size: int, out_size: int):
    """ATen anti-aliased bilinear tap table (host numpy): (first, count, weights [out_size, kmax])."""
    lib = load_library()
    kmax = lib.imcui_hip_aa_table(in_size, out_size, None, None, None, 0)
    if kmax <= 0:
        raise ImcuiHipError(f"aa table {in_size} -> {out_size}")
    first, count = np.zeros(out_size, dtype=np.int32), np.zeros(out_size, dtype=np.int32)
    w = np.zeros((out_size, kmax), dtype=np.float32)
    if lib.imcui_hip_aa_table(in_size, out_size, first.ctypes.data, count.ctypes.data, w.ctypes.data, kmax) != kmax:
        raise ImcuiHipError(f"aa table {in_size} -> {out_size}")
    return first, count, w


def preprocess_linear(img_u8: torch.Tensor, size) -> torch.Tensor:
    """Device-side `resize_image(..., "cv2_area")` when a side GROWS (extract_features.py:29-31: cv2.INTER_LINEAR): uint8
    [B,H,W] / [B,H,W,C] on the device -> gray (cv2 fixed point) -> float32 -> INTER_LINEAR to `size` = (w, h) -> / 255 ->
    float32 [B,1,h,w]."""
    if img_u8.dtype != torch.uint8 or img_u8.dim() not in (3, 4):
        raise ImcuiHipError("preprocess_linear expects uint8 [B,H,W] or [B,H,W,C]")
    if img_u8.dim() == 3:
        img_u8 = img_u8[..., None]
    hd = get_handle(img_u8.device)
    img_u8 = img_u8.contiguous()
    B, H, W, Cc = img_u8.shape
    ow, oh = int(size[0]), int(size[1])
    key = (W, ow, H, oh, str(img_u8.device))
    if key not in _linear_tables:
        _linear_tables[key] = tuple(torch.from_numpy(a).to(img_u8.device) for a in (*linear_table_host(W, ow, True), *linear_table_host(H, oh, False)))
    tabs = _linear_tables[key]
    out = torch.empty((B, 1, oh, ow), dtype=torch.float32, device=img_u8.device)
    hd.launch(hd.lib.imcui_hip_preprocess_linear_f32, _ptr(img_u8), B, H, W, Cc, *[_ptr(t) for t in tabs], _ptr(out), oh, ow)
    return out


def resize_aa(image: torch.Tensor, size_hw) -> torch.Tensor:
    """Device-side `torchvision.transforms.functional.resize(image, size, antialias=True)` of a float image [..., H, W]
    (extract_features.py:142-148, match_dense.py:182): ATen's anti-aliased bilinear arithmetic, bit for bit.  Like torchvision,
    returns the image unchanged when the size already matches."""
    oh, ow = int(size_hw[0]), int(size_hw[1])
    H, W = image.shape[-2:]
    if (oh, ow) == (H, W):
        return image
    hd = get_handle(image.device)
    src = image.contiguous().float()
    planes = src.numel() // (H * W)
    key = (W, ow, H, oh, str(image.device))
    if key not in _aa_tables:
        xt, yt = aa_table_host(W, ow), aa_table_host(H, oh)
        _aa_tables[key] = (tuple(torch.from_numpy(a).to(image.device) for a in xt), xt[2].shape[1], tuple(torch.from_numpy(a).to(image.device) for a in yt), yt[2].shape[1])
    xt, kx, yt, ky = _aa_tables[key]
    out = torch.empty((*src.shape[:-2], oh, ow), dtype=torch.float32, device=image.device)
    hd.launch(hd.lib.imcui_hip_resize_aa_f32, _ptr(src), planes, H, W, _ptr(xt[0]), _ptr(xt[1]), _ptr(xt[2]), kx, _ptr(yt[0]), _ptr(yt[1]),
              _ptr(yt[2]), ky, _ptr(out), oh, ow)  # fmt: skip
    return out


def pack_linear_split(w: torch.Tensor):
    """Host: nn.Linear weight [N, K] -> (hi, lo) uint16 fragment-major planes and the inverse scale 2^-e."""
    lib = load_library()
    wh = _as_f32_host(w)
    N, K = wh.shape
    npad = (N + 31) // 32 * 32
    hi = np.zeros(npad * K, dtype=np.uint16)
    lo = np.zeros(npad * K, dtype=np.uint16)
    sc = lib.imcui_hip_linear_pack_split(wh.ctypes.data, N, K, hi.ctypes.data, lo.ctypes.data)
    if sc <= 0:
        raise ImcuiHipError("linear_pack_split failed (K must be a multiple of 16)")
    return hi, lo, float(sc)


def linear_split_f32(a: torch.Tensor, w: torch.Tensor, bias: torch.Tensor | None, relu: bool = False) -> torch.Tensor:
    """Building block: a projection with PRE-SPLIT weights, i.e. the GEMM path every network layer takes in the split
    mode (fragment-major planes, 128- or 256-column tiles by N)."""
    hd = get_handle(a.device)
    a = a.contiguous().float()
    M, K = a.shape
    N = w.shape[0]
    hi, lo, sc = pack_linear_split(w)
    dh = torch.from_numpy(hi.view(np.int16)).to(a.device)
    dl = torch.from_numpy(lo.view(np.int16)).to(a.device)
    ds = torch.tensor([sc], dtype=torch.float32, device=a.device)
    c = torch.empty((M, N), dtype=torch.float32, device=a.device)
    hd.launch(hd.lib.imcui_hip_linear_split_f32, _ptr(a), _ptr(dh), _ptr(dl), _ptr(ds), _ptr(bias), _ptr(c), M, N, K, int(relu))
    return c


def set_range_check(device, enable: bool = True) -> None:
    """Debugging aid: scan the f32 activation operand of every split-mode GEMM / convolution / FFN launch for values the f16
    split cannot carry (imcui_hip_set_range_check)."""
    hd = get_handle(torch.device(device))
    hd.call(hd.lib.imcui_hip_set_range_check, int(bool(enable)))


def range_status(device) -> int:
    """Accumulated range-check word since the last read (synchronises): bit 0 = |x| > 65504 seen, bit 1 = NaN / Inf seen."""
    hd = get_handle(torch.device(device))
    st = C.c_int(0)
    hd.call(hd.lib.imcui_hip_get_range_status, C.byref(st))
    return int(st.value)


def qkv_split_f32(x: torch.Tensor, w: torch.Tensor, bias, cos, sin, cnt: torch.Tensor, rows_per_seq: int, alpha: float, cross: bool = False):
    """Building block: the attention-layout projection (imcui_hip_qkv_split_f32).  x [nseq * R, 256] (device), w [768 | 512, 256]
    (host, packed row order) -> int16 views of the planes: q, k [2, nseq, 4, R, 64], vt [2, nseq, 4, 64, R] (plane 0 = hi)."""
    hd = get_handle(x.device)
    x = x.contiguous().float()
    R = int(rows_per_seq)
    nseq = x.shape[0] // R
    hi, lo, sc = pack_linear_split(w)
    dev = x.device
    dh = torch.from_numpy(hi.view(np.int16)).to(dev)
    dl = torch.from_numpy(lo.view(np.int16)).to(dev)
    ds = torch.tensor([sc], dtype=torch.float32, device=dev)
    q = torch.zeros((2, nseq, 4, R, 64), dtype=torch.int16, device=dev)
    k = torch.zeros((2, nseq, 4, R, 64), dtype=torch.int16, device=dev)
    v = torch.zeros((2, nseq, 4, 64, R), dtype=torch.int16, device=dev)
    cnt = cnt.to(torch.int32).contiguous()
    hd.launch(hd.lib.imcui_hip_qkv_split_f32, _ptr(x), _ptr(dh), _ptr(dl), _ptr(ds), _ptr(bias), _ptr(cos), _ptr(sin), _ptr(cnt), nseq, R,
              float(alpha), int(cross), _ptr(q), _ptr(k), _ptr(v))  # fmt: skip
    return q, k, v


def pack_ffn_w2(w2: torch.Tensor):
    """Host: ffn.3 weight [256, 512] -> planes in the K order of the fused FFN kernel, and the inverse scale."""
    lib = load_library()
    wh = _as_f32_host(w2)
    assert wh.shape == (256, 512)
    hi = np.zeros(256 * 512, dtype=np.uint16)
    lo = np.zeros(256 * 512, dtype=np.uint16)
    sc = lib.imcui_hip_ffn_pack_w2(wh.ctypes.data, hi.ctypes.data, lo.ctypes.data)
    if sc <= 0:
        raise ImcuiHipError("ffn_pack_w2 failed")
    return hi, lo, float(sc)


class FusedFFN:
    """Building block: x + W2 GELU(LN(W1 [x | ctx] + b1)) + b2 in ONE kernel (csrc/ffn.hip), weights packed once.
    gamma = beta = None: ReLU instead of LayerNorm + GELU (SuperGlue's MLP with the BatchNorm folded into W1, b1).
    act = 2 / 3: x + LN_256(W2 act(W1 [x | ctx] + b1) + b2) with LeakyReLU(0.01) / ReLU (gamma, beta [256]): the dense matchers."""

    def __init__(self, w1, b1, gamma, beta, w2, b2, device, act=None):
        self.act = act if act is not None else (1 if gamma is None else 0)
        if gamma is None:
            gamma = beta = torch.zeros(512)
        def up(a):
            return torch.from_numpy(a.view(np.int16)).to(device)

        h1, l1, s1 = pack_linear_split(w1)
        h2, l2, s2 = pack_ffn_w2(w2)
        self.w1h, self.w1l, self.w2h, self.w2l = up(h1), up(l1), up(h2), up(l2)
        self.s1 = torch.tensor([s1], dtype=torch.float32, device=device)
        self.s2 = torch.tensor([s2], dtype=torch.float32, device=device)
        self.b1, self.gamma, self.beta, self.b2 = (t.detach().float().contiguous().to(device) for t in (b1, gamma, beta, b2))

    def __call__(self, x: torch.Tensor, ctx: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        hd = get_handle(x.device)
        x, ctx = x.contiguous().float(), ctx.contiguous().float()
        M = x.shape[0]
        out = torch.empty_like(x) if out is None else out
        hd.launch(hd.lib.imcui_hip_ffn_split_f32, _ptr(x), _ptr(ctx), _ptr(self.w1h), _ptr(self.w1l), _ptr(self.s1), _ptr(self.b1), _ptr(self.gamma),
                  _ptr(self.beta), _ptr(self.w2h), _ptr(self.w2l), _ptr(self.s2), _ptr(self.b2), _ptr(out), M, self.act)  # fmt: skip
        return out


def conv3x3_f32(x_nhwc: torch.Tensor, w_oihw: torch.Tensor, bias: torch.Tensor, relu=True, pool=False) -> torch.Tensor:
    hd = get_handle(x_nhwc.device)
    lib = hd.lib
    B, H, W, Cin = x_nhwc.shape
    Cout = w_oihw.shape[0]
    wh = _as_f32_host(w_oihw)
    x_nhwc = x_nhwc.contiguous().float()
    bias = bias.contiguous().float().to(x_nhwc.device)
    out = torch.empty((B, H // 2, W // 2, Cout) if pool else (B, H, W, Cout), dtype=torch.float32, device=x_nhwc.device)
    if lib.imcui_hip_get_precision(hd.h) == 1:
        hi = np.zeros(Cout * Cin * 9, dtype=np.uint16)
        lo = np.zeros(Cout * Cin * 9, dtype=np.uint16)
        sc = lib.imcui_hip_conv3x3_pack_split(wh.ctypes.data, Cout, Cin, hi.ctypes.data, lo.ctypes.data)
        if sc == 0.0:
            raise ImcuiHipError("conv3x3_pack_split failed")
        dh = torch.from_numpy(hi.view(np.int16)).to(x_nhwc.device)
        dl = torch.from_numpy(lo.view(np.int16)).to(x_nhwc.device)
        ds = torch.tensor([sc], dtype=torch.float32, device=x_nhwc.device)
        hd.launch(lib.imcui_hip_conv3x3_split_f32, _ptr(x_nhwc), _ptr(dh), _ptr(dl), _ptr(ds), _ptr(bias), _ptr(out), B, H, W, Cin, Cout, int(relu), int(pool))
        return out
    packed = np.zeros(Cout * Cin * 9, dtype=np.float32)
    if lib.imcui_hip_conv3x3_pack(wh.ctypes.data, Cout, Cin, packed.ctypes.data) != 0:
        raise ImcuiHipError("conv3x3_pack failed")
    wp = torch.from_numpy(packed).to(x_nhwc.device)
    hd.launch(lib.imcui_hip_conv3x3_f32, _ptr(x_nhwc), _ptr(wp), _ptr(bias), _ptr(out), B, H, W, Cin, Cout, int(relu), int(pool))
    return out


# ------------------------------------------------------------------ the shared GEMM, entered directly (kernel-variant tests)
GEMM_EPI = {"bias": 0, "relu": 1, "resid": 2, "qkv": 3, "cross": 4, "conv": 5, "qkv_vit": 7, "nnstat": 8}
# GemmRouteKind of csrc/gemm.h: a route is 16 kind + epilogue (imcui_hip_gemm_last_route)
GEMM_ROUTE_KINDS = {"none": 0, "exact": 1, "split_f32b": 2, "split_128": 3, "split_256": 4, "split_128_single": 5, "split_256_single": 6,
                    "conv_f32b": 7, "conv_128": 8, "conv_256": 9, "conv_128_single": 10, "conv_256_single": 11, "wreg_rolled": 12,
                    "wreg_pipe": 13, "wreg_rolled_single": 14, "wreg_pipe_single": 15, "wreg_mt2": 16, "wreg_mt1": 17,
                    "exact_dil": 18, "convd_f32b": 19, "convd_128": 20, "convd_256": 21}  # fmt: skip
# GemmFeature of csrc/gemm.h: what a launch ran with besides its route (imcui_hip_gemm_route_features)
GEMM_FEATURES = {"conv_k1": 1 << 0, "conv_k3": 1 << 1, "conv_k5": 1 << 2, "conv_kother": 1 << 3, "stride2": 1 << 4, "stride_other": 1 << 5,
                 "pad_not_same": 1 << 6, "dilated": 1 << 7, "chunk": 1 << 8, "long_k": 1 << 9, "resid": 1 << 10, "rup": 1 << 11,
                 "act1": 1 << 12, "act2": 1 << 13, "act3": 1 << 14, "ldc": 1 << 15, "n_mod32": 1 << 16, "n_mod_tile": 1 << 17,
                 "m_small": 1 << 18, "a2": 1 << 19, "batch": 1 << 20, "mcnt": 1 << 21, "ncnt": 1 << 22, "conv_batched": 1 << 23,
                 "cnt": 1 << 24, "active": 1 << 25, "wsel": 1 << 26, "ln": 1 << 27, "alpha": 1 << 28, "no_bias": 1 << 29,
                 "group_rows": 1 << 30}  # fmt: skip
GEMM_CHUNK_MIN_K = 2048  # gemm.h: dilated launches sum in two levels from this K on, and K >= this is a "long" sum (long_k / chunk)
GEMM_EXACT_CHUNK_MIN_K = 4096  # gemm.h: undilated launches of the exact kernel sum in two levels from this K on
GEMM_WIDE_KINDS = ("split_256", "split_256_single", "conv_256", "conv_256_single", "convd_256", "wreg_rolled", "wreg_pipe",
                   "wreg_rolled_single", "wreg_pipe_single", "wreg_mt2", "wreg_mt1")  # 256-column tiles; every other kind: 128


def gemm_route(kind: str, epi: str) -> int:
    return GEMM_ROUTE_KINDS[kind] * 16 + GEMM_EPI[epi]


def gemm_route_name(route: int) -> str:
    kinds = {v: k for k, v in GEMM_ROUTE_KINDS.items()}
    epis = {v: k for k, v in GEMM_EPI.items()}
    return f"{kinds.get(route // 16, route // 16)}/{epis.get(route % 16, route % 16)}"


class GemmDesc(C.Structure):
    """imcui_hip_gemm_desc, laid out from include/imcui_hip.h."""

    _fields_ = _desc_fields("imcui_hip_gemm_desc")
    DEFAULTS = {"batch": 1, "cnt_stride": 1, "conv_stride": 1, "rup_align": 1, "heads": 4, "alpha": 1.0}


class GemmWeights:
    """One or more weight sets [N, K] (host) in both operand formats of the GEMM, on `device`: f32 rows (W, set stride in floats) and the
    pre-split fragment-major planes of pack_linear_split (Wh / Wl, set stride in halves; wscale[set] = that set's 2^-e)."""

    def __init__(self, sets, device):
        sets = [_as_f32_host(w) for w in sets]
        self.N, self.K = sets[0].shape
        packs = [pack_linear_split(w) for w in sets]
        self.W = torch.from_numpy(np.concatenate([w.reshape(-1) for w in sets])).to(device)
        self.Wh = torch.from_numpy(np.concatenate([p[0] for p in packs]).view(np.int16)).to(device)
        self.Wl = torch.from_numpy(np.concatenate([p[1] for p in packs]).view(np.int16)).to(device)
        self.wscale = torch.tensor([p[2] for p in packs], dtype=torch.float32, device=device)
        self.f32_stride, self.half_stride = self.N * self.K, packs[0][0].size

    @classmethod
    def conv(cls, w_oihw_sets, device):
        """OIHW convolution weights -> the GEMM weight [Cout][tap][Cin] of the implicit im2col (_conv_gemm_layout)."""
        mats = []
        for w in w_oihw_sets:
            w = w.float().cpu()
            mats.append(_conv_gemm_layout(w, torch.zeros(w.shape[0]), w.shape[0], w.shape[1])[0])
        return cls(mats, device)

    def fields(self, split: bool, planes: bool = True) -> dict:
        """Descriptor fields of this operand: the planes (split mode, `planes`) or the f32 rows; w_stride in the matching unit."""
        if split and planes:
            return {"Wh": self.Wh, "Wl": self.Wl, "wscale": self.wscale, "W": self.W, "ldw": self.K, "w_stride": self.half_stride}
        return {"W": self.W, "ldw": self.K, "wscale": self.wscale, "w_stride": self.f32_stride}


def gemm_probe(device: torch.device, check: bool = True, **fields) -> int:
    """One launch through gemm_launch (imcui_hip_gemm_probe_f32) with the descriptor `fields` (tensors become device pointers, `epi`
    may be a GEMM_EPI name).  Returns the route of the launch (GEMM_ROUTE_KINDS); with check=False a refused call returns its
    negative status instead of raising."""
    hd = get_handle(device)
    fields = {**GemmDesc.DEFAULTS, **fields}
    if isinstance(fields.get("epi"), str):
        fields["epi"] = GEMM_EPI[fields["epi"]]
    d = _fill_desc(GemmDesc(), fields, "gemm_probe")
    rc = hd.launch(hd.lib.imcui_hip_gemm_probe_f32, C.byref(d), check=check)
    return rc if rc != 0 else int(hd.lib.imcui_hip_gemm_last_route(hd.h))


def gemm_route_counts(device: torch.device) -> dict:
    """{route: launches} of every GEMM launch on the device's handle since gemm_route_reset."""
    return _route_table(device, "imcui_hip_gemm_route_counts")


def gemm_route_features(device: torch.device) -> dict:
    """{route: OR of the GEMM_FEATURES bits its launches ran with} since gemm_route_reset (routes with no feature are absent)."""
    return _route_table(device, "imcui_hip_gemm_route_features")


def gemm_feature_names(mask: int) -> list:
    return [k for k, v in GEMM_FEATURES.items() if mask & v]


def gemm_route_reset(device: torch.device) -> None:
    hd = get_handle(device)
    hd.call(hd.lib.imcui_hip_gemm_route_reset)


# ------------------------------------------------------------------ the attention launcher, entered directly (kernel-variant tests)
# AttnRouteKind of csrc/attention.h: a route is 2 kind + split (imcui_hip_attn_last_route); split = 1: the key-split launch + combine
ATTN_ROUTE_KINDS = {"none": 0, "exact": 1, "natlog": 2, "l2d_v8": 3, "l2d_v7": 4, "l2d_single": 5, "mx": 6}


def attn_route(kind: str, split: bool = False) -> int:
    return ATTN_ROUTE_KINDS[kind] * 2 + int(bool(split))


def attn_route_name(route: int) -> str:
    kinds = {v: k for k, v in ATTN_ROUTE_KINDS.items()}
    return f"{kinds.get(route // 2, route // 2)}{'/split' if route % 2 else ''}"


class AttnDesc(C.Structure):
    """imcui_hip_attn_desc, laid out from include/imcui_hip.h."""

    _fields_ = _desc_fields("imcui_hip_attn_desc")
    DEFAULTS = {"heads": 4, "variant": -1}


def attention_probe(device: torch.device, check: bool = True, **fields) -> int:
    """One launch through attention_launch (imcui_hip_attention_probe_f32) with the descriptor `fields` (tensors become device pointers;
    V6_bytes / part_bytes default to the sizes of the tensors given as V6 / part).  Returns the route of the launch (ATTN_ROUTE_KINDS);
    with check=False a refused call returns its negative status instead of raising."""
    hd = get_handle(device)
    fields = {**AttnDesc.DEFAULTS, **fields}
    for k in ("V6", "part"):
        if isinstance(fields.get(k), torch.Tensor):
            fields.setdefault(k + "_bytes", fields[k].numel() * fields[k].element_size())
    d = _fill_desc(AttnDesc(), fields, "attention_probe")
    rc = hd.launch(hd.lib.imcui_hip_attention_probe_f32, C.byref(d), check=check)
    return rc if rc != 0 else int(hd.lib.imcui_hip_attn_last_route(hd.h))


def attention_part_floats(device: torch.device, S: int, heads: int, rows: int) -> int:
    return int(get_handle(device).lib.imcui_hip_attention_part_floats(S, heads, rows))


def attn_route_counts(device: torch.device) -> dict:
    """{route: launches} of every attention launch on the device's handle since attn_route_reset."""
    return _route_table(device, "imcui_hip_attn_route_counts")


def attn_route_reset(device: torch.device) -> None:
    hd = get_handle(device)
    hd.call(hd.lib.imcui_hip_attn_route_reset)


# ------------------------------------------------------------------ the fused-FFN launcher, entered directly (kernel-variant tests)
# FfnRouteKind of csrc/ffn.h: a route is 1 + 4 kind + act (imcui_hip_ffn_last_route); 0 = nothing launched
FFN_ROUTE_KINDS = {"t128_rolled": 0, "t128": 1, "t64": 2, "t32": 3}


def ffn_route(kind: str, act: int) -> int:
    return 1 + FFN_ROUTE_KINDS[kind] * 4 + int(act)


def ffn_route_name(route: int) -> str:
    if route <= 0:
        return "none"
    kinds = {v: k for k, v in FFN_ROUTE_KINDS.items()}
    return f"{kinds.get((route - 1) // 4, (route - 1) // 4)}/act{(route - 1) % 4}"


class FfnDesc(C.Structure):
    """imcui_hip_ffn_desc, laid out from include/imcui_hip.h."""

    _fields_ = _desc_fields("imcui_hip_ffn_desc")


class FfnWeights:
    """The two Linear layers of one FFN (host W1 [512, 512], W2 [256, 512]) in the operand format of csrc/ffn.hip, packed once and kept on
    `device`: W1 as the planes of pack_linear_split, W2 as the planes of pack_ffn_w2 (K axis in the kernel's hand-over order), each with
    its 2^-e scale.  The host copies of the planes and scales stay available (w1_planes / w2_planes: what the kernel multiplies)."""

    def __init__(self, w1, w2, device):
        self.w1_planes = pack_linear_split(w1)
        self.w2_planes = pack_ffn_w2(w2)

        def up(a):
            return torch.from_numpy(a.view(np.int16)).to(device)

        self.w1h, self.w1l, self.w2h, self.w2l = up(self.w1_planes[0]), up(self.w1_planes[1]), up(self.w2_planes[0]), up(self.w2_planes[1])
        self.s1 = torch.tensor([self.w1_planes[2]], dtype=torch.float32, device=device)
        self.s2 = torch.tensor([self.w2_planes[2]], dtype=torch.float32, device=device)

    def fields(self) -> dict:
        return {"w1h": self.w1h, "w1l": self.w1l, "s1": self.s1, "w2h": self.w2h, "w2l": self.w2l, "s2": self.s2}


def ffn_probe(device: torch.device, check: bool = True, **fields) -> int:
    """One launch through ffn_launch (imcui_hip_ffn_probe_f32) with the descriptor `fields` (tensors become device pointers, None a null
    pointer).  Returns the route of the launch (ffn_route); with check=False a refused call returns its negative status instead of
    raising."""
    hd = get_handle(device)
    d = _fill_desc(FfnDesc(), fields, "ffn_probe")
    rc = hd.launch(hd.lib.imcui_hip_ffn_probe_f32, C.byref(d), check=check)
    return rc if rc != 0 else int(hd.lib.imcui_hip_ffn_last_route(hd.h))


def ffn_route_counts(device: torch.device) -> dict:
    """{route: launches} of every fused-FFN launch on the device's handle since ffn_route_reset."""
    return _route_table(device, "imcui_hip_ffn_route_counts")


def ffn_route_reset(device: torch.device) -> None:
    hd = get_handle(device)
    hd.call(hd.lib.imcui_hip_ffn_route_reset)


# ------------------------------------------------------------------ the 3x3 convolution launchers, entered directly (kernel-variant tests)
# ConvRouteKind / ConvFeature of csrc/conv.h (imcui_hip_conv_last_route, imcui_hip_conv_route_features)
CONV_ROUTE_KINDS = {"none": 0, "f32": 1, "split_n2": 2, "split_n4": 3, "split_n2_single": 4, "split_n4_single": 5, "tall": 6,
                    "tall_single": 7, "fused_8row": 8, "fused_tall": 9, "conv1a": 10}  # fmt: skip
CONV_FEATURES = {"pool": 1, "resid": 2, "resid2": 4, "leaky": 8, "relu_in": 16, "cin_stride": 32, "cout_live": 64, "head": 128,
                 "head_no_out": 256, "head_raw": 512}  # fmt: skip
CONV_ENTRIES = {"f32": 0, "split": 1, "fused": 2, "conv1a": 3}


def conv_route(kind: str) -> int:
    return CONV_ROUTE_KINDS[kind]


def conv_route_name(route: int) -> str:
    return {v: k for k, v in CONV_ROUTE_KINDS.items()}.get(route, str(route))


def conv_feature_names(mask: int) -> list:
    return [k for k, v in CONV_FEATURES.items() if mask & v]


class ConvDesc(C.Structure):
    """imcui_hip_conv_desc, laid out from include/imcui_hip.h."""

    _fields_ = _desc_fields("imcui_hip_conv_desc")


class ConvWeights:
    """A 3x3 layer (host OIHW weights, bias) in the operand formats of csrc/conv.hip, on `device`: the packed f32 layout of
    conv3x3_kernel (wp), the pre-split f16 hi / lo planes of w * 2^e (wh / wl) with wscale = 2^-e, and the bias.
    cout_pad: the layer is zero-padded to that many output channels (zero weights and bias: what cout_live skips);
    cin_used: only the first cin_used input channels are packed (the stored map has more: cin_stride)."""

    def __init__(self, w_oihw, bias, device, cout_pad=None, cin_used=None):
        w = torch.as_tensor(w_oihw).float().cpu()
        b = torch.as_tensor(bias).float().cpu()
        if cin_used is not None:
            w = w[:, :cin_used]
        if cout_pad is not None and cout_pad > w.shape[0]:
            w = torch.cat([w, torch.zeros(cout_pad - w.shape[0], *w.shape[1:])])
            b = torch.cat([b, torch.zeros(cout_pad - b.shape[0])])
        self.Cout, self.Cin = w.shape[0], w.shape[1]
        if self.Cin % 32 or self.Cout % 64 or tuple(w.shape[2:]) != (3, 3):
            raise ImcuiHipError(f"ConvWeights: [{self.Cout}, {self.Cin}, {tuple(w.shape[2:])}] is no layer of conv.hip (Cin % 32, Cout % 64, 3x3)")
        lib = load_library()
        wh = _as_f32_host(w)
        n = self.Cout * self.Cin * 9
        packed, hi, lo = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.uint16), np.zeros(n, dtype=np.uint16)
        if lib.imcui_hip_conv3x3_pack(wh.ctypes.data, self.Cout, self.Cin, packed.ctypes.data) != 0:
            raise ImcuiHipError("conv3x3_pack failed")
        self.scale = float(lib.imcui_hip_conv3x3_pack_split(wh.ctypes.data, self.Cout, self.Cin, hi.ctypes.data, lo.ctypes.data))
        if self.scale == 0.0:
            raise ImcuiHipError("conv3x3_pack_split failed")
        self.w_oihw, self.bias_host, self.packed_host, self.hi_host, self.lo_host = w, b, packed, hi, lo
        self.wp = torch.from_numpy(packed).to(device)
        self.wh = torch.from_numpy(hi.view(np.int16)).to(device)
        self.wl = torch.from_numpy(lo.view(np.int16)).to(device)
        self.wscale = torch.tensor([self.scale], dtype=torch.float32, device=device)
        self.bias = b.to(device)

    @staticmethod
    def first_layer(w_oihw) -> torch.Tensor:
        """[64, 1, 3, 3] -> [9 taps][64] (pack_conv1a), host."""
        return torch.as_tensor(w_oihw).float().cpu().reshape(64, 9).t().contiguous()

    def fields(self, split: bool) -> dict:
        if split:
            return {"wh": self.wh, "wl": self.wl, "wscale": self.wscale, "bias": self.bias}
        return {"wp": self.wp, "bias": self.bias}


def conv_probe(device: torch.device, check: bool = True, **fields) -> int:
    """One launch through a launcher of csrc/conv.h (imcui_hip_conv_probe_f32) with the descriptor `fields` (tensors become device
    pointers, `entry` may be a CONV_ENTRIES name).  Returns the route of the launch (CONV_ROUTE_KINDS); with check=False a refused call
    returns its negative status instead of raising."""
    hd = get_handle(device)
    if isinstance(fields.get("entry"), str):
        fields["entry"] = CONV_ENTRIES[fields["entry"]]
    d = _fill_desc(ConvDesc(), fields, "conv_probe")
    rc = hd.launch(hd.lib.imcui_hip_conv_probe_f32, C.byref(d), check=check)
    return rc if rc != 0 else int(hd.lib.imcui_hip_conv_last_route(hd.h))


def conv_route_counts(device: torch.device) -> dict:
    """{route: launches} of every launch of csrc/conv.hip on the device's handle since conv_route_reset."""
    return _route_table(device, "imcui_hip_conv_route_counts")


def conv_route_features(device: torch.device) -> dict:
    """{route: OR of the CONV_FEATURES bits its launches ran with} since conv_route_reset (routes with no feature are absent)."""
    return _route_table(device, "imcui_hip_conv_route_features")


def conv_route_reset(device: torch.device) -> None:
    hd = get_handle(device)
    hd.call(hd.lib.imcui_hip_conv_route_reset)


def _split_planes(t: torch.Tensor) -> torch.Tensor:
    """f32 tensor -> [2, ...] f16 (hi, lo) planes, the operand format of the split attention kernel."""
    hi = t.half()
    lo = (t - hi.float()).half()
    return torch.stack([hi, lo], 0).contiguous()


def attention_f32(q, k, v, cnt, cross=False, log2_domain=False):
    """q,k,v [S,heads,rows,64] head-major (q pre-scaled); cnt [S] int32 -> [S*rows, heads*64].
    log2_domain: q is multiplied by log2(e) here and the kernel's base-2 soft-max path (the one the layers use) runs."""
    hd = get_handle(q.device)
    S, Hh, R, d = q.shape
    assert d == 64
    if log2_domain:
        q = q.float() * 1.4426950408889634
    if hd.lib.imcui_hip_get_precision(hd.h) == 1:
        # the split kernel consumes pre-split f16 planes of Q, K and V^T [S,heads,64,rows]
        q, k, v = _split_planes(q.float()), _split_planes(k.float()), _split_planes(v.float().transpose(2, 3).contiguous())
    else:
        q, k, v = q.contiguous().float(), k.contiguous().float(), v.contiguous().float()
    o = torch.zeros((S * R, Hh * 64), dtype=torch.float32, device=q.device)
    cnt = cnt.to(torch.int32).contiguous()
    hd.launch(hd.lib.imcui_hip_attention_f32, _ptr(q), _ptr(k), _ptr(v), _ptr(o), _ptr(cnt), S, Hh, R, int(cross), int(bool(log2_domain)))
    return o


def attention_mx_f32(q, k, v, cnt, cross=False):
    """`attention_f32(..., log2_domain=True)` in attention variant 9 (csrc/attention_mx.hip: P.V as one f16 product + two block-scaled fp6
    correction products); split arithmetic only."""
    hd = get_handle(q.device)
    S, Hh, R, d = q.shape
    assert d == 64
    q = _split_planes(q.float() * 1.4426950408889634)
    k, v = _split_planes(k.float()), _split_planes(v.float().transpose(2, 3).contiguous())
    o = torch.zeros((S * R, Hh * 64), dtype=torch.float32, device=q.device)
    cnt = cnt.to(torch.int32).contiguous()
    nbytes = hd.lib.imcui_hip_attention_mx_scratch_bytes(S, Hh, R)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=q.device)
    hd.launch(hd.lib.imcui_hip_attention_mx_f32, _ptr(q), _ptr(k), _ptr(v), _ptr(o), _ptr(cnt), S, Hh, R, int(cross), _ptr(scratch), nbytes)
    return o


# ------------------------------------------------------------------ the list-building blocks of csrc/select.h, entered directly
SELECT_OPS = {"compact": 0, "scan": 1, "order_key": 2, "kth32": 3, "kth64": 4, "rank4": 5, "rank16": 6, "keep": 7, "cut": 8}
SELECT_MAXB = header.read().defines["IMCUI_SELECT_MAXB"]
SELECT_RULES = {1: "op", 2: "B", 3: "n / capacity", 4: "k", 5: "cap / limit", 6: "null pointer", 7: "nlev"}  # imcui_hip_select_desc_check


class SelectDesc(C.Structure):
    """imcui_hip_select_desc, laid out from include/imcui_hip.h."""

    _fields_ = _desc_fields("imcui_hip_select_desc")


def select_desc(**fields) -> SelectDesc:
    """A SelectDesc from `fields`: tensors become their data pointers, `op` may be a SELECT_OPS name, n_row / k_row take sequences."""
    d = SelectDesc()
    for k, v in fields.items():
        if k == "op" and isinstance(v, str):
            v = SELECT_OPS[v]
        if k in ("n_row", "k_row"):
            v = [int(x) for x in v]
            if len(v) > SELECT_MAXB:
                raise ImcuiHipError(f"select_desc: {k} holds at most {SELECT_MAXB} rows")
            v = (C.c_int * SELECT_MAXB)(*v)
        elif isinstance(v, torch.Tensor):
            v = v.data_ptr()
        elif v is None:
            v = 0
        setattr(d, k, v)
    return d


def select_probe(device: torch.device, check: bool = True, **fields) -> int:
    """One op of imcui_hip_select_probe with the descriptor `fields` (device tensors become pointers).  Returns 0; with check=False a
    refused call returns its negative status instead of raising."""
    hd = get_handle(device)
    for k, v in fields.items():
        if isinstance(v, torch.Tensor) and v.device.type != "cuda":
            raise ImcuiHipError(f"select_probe: field {k} must be a device tensor")
    d = select_desc(**fields)
    return int(hd.launch(hd.lib.imcui_hip_select_probe, C.byref(d), check=check))


def simple_nms(scores: torch.Tensor, radius: int) -> torch.Tensor:
    hd = get_handle(scores.device)
    scores = scores.contiguous().float()
    B, H, W = scores.shape
    out = torch.empty_like(scores)
    hd.launch(hd.lib.imcui_hip_simple_nms, _ptr(scores), _ptr(out), B, H, W, int(radius))
    return out
