"""torch CUDA tensors at the C-ABI's device entries (include/of2d.h,
``of2d_darray``): a tensor is handed over by pointer, strides and dtype, never
copied, and the call is ordered with the current stream of the tensor's device.

torch is imported lazily: a caller that passes a torch tensor has imported it.
Everything here raises ``ValueError`` before the library is entered.
"""
from __future__ import annotations

import ctypes as C
import sys

from . import _lib


def _torch():
    import torch
    return torch


def is_cuda(a) -> bool:
    """A torch tensor on a GPU (anything else takes the host path)."""
    torch = sys.modules.get("torch")
    return torch is not None and isinstance(a, torch.Tensor) and a.is_cuda


def all_cuda(**arrays) -> bool:
    """True when every argument is a CUDA tensor, False when none is; a mix is
    a ``ValueError``, and so are CUDA tensors of different devices."""
    flags = {k: is_cuda(v) for k, v in arrays.items()}
    if not any(flags.values()):
        return False
    if not all(flags.values()):
        host = ", ".join(k for k, f in flags.items() if not f)
        raise ValueError(f"CUDA tensors and host arrays in one call ({host} is not a CUDA tensor)")
    devs = {v.device for v in arrays.values()}
    if len(devs) > 1:
        raise ValueError(f"CUDA tensors of different devices in one call: {sorted(map(str, devs))}")
    return True


def _dtype_code(t, name: str) -> int:
    torch = _torch()
    if t.dtype == torch.float32:
        return _lib.OF2D_F32
    if t.dtype == torch.float64:
        return _lib.OF2D_F64
    raise ValueError(f"{name} is {t.dtype}, expected torch.float32 or torch.float64")


def darray(t, shape, axes, name: str) -> _lib.DArray:
    """The ``of2d_darray`` of tensor ``t`` of exactly ``shape``; ``axes[d]`` is
    the of2d_darray axis (0 pair, 1 x, 2 y, 3 component) of dimension ``d``."""
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} is {tuple(t.shape)}, expected {tuple(shape)}")
    a = _lib.DArray()
    a.dtype = _dtype_code(t, name)
    a.ptr = t.data_ptr()
    for d, ax in enumerate(axes):
        a.stride[ax] = t.stride(d)
    return a


def stream_of(t) -> C.c_void_p:
    """The current stream of the tensor's device, as the entries' ``stream``."""
    return C.c_void_p(_torch().cuda.current_stream(t.device).cuda_stream)


def output(out, shape, dtype, device, name: str = "out"):
    """``out`` checked, or a new tensor of ``shape`` on ``device`` (a
    ``torch.device``, an index, or ``None`` for the current CUDA device)."""
    torch = _torch()
    if out is None:
        dtype = torch.float32 if dtype is None else dtype
        if dtype not in (torch.float32, torch.float64):
            raise ValueError(f"dtype is {dtype}, expected torch.float32 or torch.float64")
        if not isinstance(device, torch.device):
            device = torch.device("cuda", torch.cuda.current_device() if device is None
                                  else int(device))
        return torch.empty(tuple(shape), dtype=dtype, device=device)
    if not is_cuda(out):
        raise ValueError(f"{name} is not a CUDA tensor")
    if tuple(out.shape) != tuple(shape):
        raise ValueError(f"{name} is {tuple(out.shape)}, expected {tuple(shape)}")
    _dtype_code(out, name)
    return out
