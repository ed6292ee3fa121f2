"""What the wrappers of the entries on a [D][H][W] volume share (surface, components, morphology, lesions): the converter
of a caller's array to a uint8 device volume, the check of an `out` tensor, and the workspace caches."""
import numpy as np
import torch

from . import _lib
from ._lib import lib, stream_ptr

_caches = []


def as_volume(a, what, dims=(2, 3), dtypes=None, who="this call needs"):
    """(uint8 [D][H][W] on the GPU, the caller's shape) from a device tensor or a numpy array (uploaded once).  dims: the
    ranks taken, a [H, W] input being the depth-1 volume [1, H, W]; dtypes: the torch dtypes taken, None for any (cast
    to uint8); who: the head of the message where there is no GPU, e.g. "surface metrics need"."""
    if not torch.cuda.is_available():
        raise _lib.HdfError(f"{who} a GPU (there is no CPU path)")
    if not torch.is_tensor(a):
        a = torch.from_numpy(np.ascontiguousarray(a))
    if a.dim() not in dims:
        forms = " or ".join(f for d, f in ((3, "[D, H, W]"), (2, "[H, W]")) if d in dims)
        raise ValueError(f"{what} must be {forms}, got {tuple(a.shape)}")
    if dtypes is not None and a.dtype not in dtypes:
        raise ValueError(f"{what} must be uint8 or bool, got {a.dtype}")
    shape = tuple(a.shape)
    if a.device.type != "cuda":
        a = a.to("cuda")
    a = a.to(torch.uint8).contiguous()
    return (a[None] if a.dim() == 2 else a), shape


def check_out(out, vol, shape):
    """the caller's `out` (None: a new tensor) as a tensor shaped like the device volume `vol`; shape: the caller's"""
    if out is None:
        return torch.empty_like(vol)
    if not (torch.is_tensor(out) and out.dtype == torch.uint8 and out.device == vol.device and out.is_contiguous()
            and tuple(out.shape) == shape):
        raise ValueError("out must be a contiguous uint8 device tensor shaped like the volume")
    return out.view(vol.shape)


class WorkspaceCache(dict):
    """(size_fn, device, stream, *args) -> uint8 tensor of lib().<size_fn>(*args) bytes: one workspace per argument tuple
    and stream.  A workspace is reused by the next call on ITS stream (the kernels of two calls are ordered there);
    callers on two streams get one each and do not race.  Nothing is evicted -- clear_all() gives the memory back."""

    def __init__(self, size_fn):
        super().__init__()
        self.size_fn = size_fn
        _caches.append(self)

    def workspace(self, dev, *args):
        key = (self.size_fn, str(dev), stream_ptr()) + args
        ws = self.get(key)
        if ws is None:
            n = getattr(lib(), self.size_fn)(*args)
            if n < 0:
                raise _lib.HdfError(self.size_fn + ": " + lib().hdf_last_error().decode(errors="replace"))
            ws = self[key] = torch.empty(n, dtype=torch.uint8, device=dev)
        return ws


def clear_all():
    """drop every cached workspace of every module"""
    for cache in _caches:
        cache.clear()
