"""ctypes binding of libimcui_hip.so (the C ABI declared in include/imcui_hip.h).

The product path fails loudly when the library is missing: there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

from . import header
from .build import LIB_PATH

_lock = threading.Lock()
_lib = None


class ImcuiHipError(RuntimeError):
    pass


# name -> (restype, argtypes) of every function include/imcui_hip.h declares, read from it: the header is the only statement of the ABI here
try:
    SIGNATURES = header.read().functions
except (OSError, header.HeaderError) as e:  # (a missing header: the OSError names the path too)
    raise ImcuiHipError(f"cannot take the ctypes signatures from {header.HEADER_PATH}: {e}") from e


def load_library(path: str | None = None):
    """dlopen the HIP backend; raises ImcuiHipError when it has not been built."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        path = path or os.environ.get("IMCUI_HIP_LIB", LIB_PATH)
        if not os.path.exists(path):
            raise ImcuiHipError(
                f"{path} not found: build it with `python __graft_entry__.py build` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback."
            )
        try:
            lib = C.CDLL(path)
        except OSError as e:  # pragma: no cover
            raise ImcuiHipError(f"cannot load {path}: {e}") from e
        for name, (res, args) in SIGNATURES.items():
            try:
                fn = getattr(lib, name)
            except AttributeError as e:
                raise ImcuiHipError(f"{path} does not export {name}") from e
            fn.restype = res
            fn.argtypes = args
        _lib = lib
        return lib
