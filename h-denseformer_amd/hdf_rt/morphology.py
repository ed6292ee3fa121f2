"""Binary morphology of a label map on the device: what scipy.ndimage.binary_dilation / binary_erosion / binary_opening /
binary_closing / binary_fill_holes do on the host after a copy of the map (117 MB for a 448x512x512 volume) and before a
copy back.  The map that sliding_window_predict returns goes through fill_class_holes or morph_class into
keep_largest_component and cal_score / multi_* without leaving the device.  Kernels: csrc/morphology.hip; definitions:
include/hdf.h.  No CPU fallback.

connectivity is 6, 18 or 26 (scipy's generate_binary_structure(3, 1 | 2 | 3)); label = 0 takes every non-zero voxel as the
mask, label = k only the voxels equal to k; border_value is what a voxel outside the volume reads as; iterations is the
number of steps, 1..256 (scipy's "until nothing changes", iterations < 1, is refused).  A [H, W] input is the depth-1
volume [1, H, W]: 6 / 18 / 26 are then the 4- / 8- / 8-neighbourhood and there is no z border.  The defaults are scipy's."""
import collections

import torch

from ._lib import check, lib, ptr, stream_ptr
from ._volume import WorkspaceCache, as_volume, check_out, clear_all

DILATE, ERODE, OPEN, CLOSE = 0, 1, 2, 3      # HDF_MORPH_*
MASK, MAP = 0, 1
OPS = {"dilate": DILATE, "erode": ERODE, "open": OPEN, "close": CLOSE}
# one workspace per entry, volume shape and stream (_volume.WorkspaceCache): a quarter of a byte a voxel for the four ops,
# about 11 bytes a voxel for fill holes, each in a cache of its own
_morph_workspaces = WorkspaceCache("hdf_morph_workspace_bytes")
_fill_workspaces = WorkspaceCache("hdf_fill_holes_workspace_bytes")
_workspaces = collections.ChainMap(_morph_workspaces, _fill_workspaces)      # both, for a reader


def clear_workspaces():
    """drop the cached workspaces: these, and those of the other entries on a volume (as hdf_rt.surface's)"""
    clear_all()


def _run(volume, out, return_counts, cache, call):
    """call(vol, dims, dst, res, ws) enqueues one entry; returns the uint8 tensor shaped like `volume` (and the counts)"""
    vol, shape = as_volume(volume, "volume", dtypes=(torch.uint8, torch.bool), who="morphology needs")
    dims = tuple(int(s) for s in vol.shape)
    dst = check_out(out, vol, shape)
    with torch.cuda.device(vol.device):
        ws = cache.workspace(vol.device, *dims)
        res = torch.empty(2, dtype=torch.int64, device=vol.device)
        call(vol, dims, dst, res, ws)
    return (dst.view(shape), res) if return_counts else dst.view(shape)


def _morph(volume, op, connectivity, iterations, label, border_value, mode, out, return_counts):
    def call(vol, dims, dst, res, ws):
        check(lib().hdf_morph(ptr(vol), int(label), int(op), int(connectivity), int(iterations), int(border_value), mode, *dims,
                              ptr(dst), ptr(res), ptr(ws), ws.numel(), stream_ptr()), "hdf_morph")
    return _run(volume, out, return_counts, _morph_workspaces, call)


def _fill(volume, connectivity, label, mode, out, return_counts):
    def call(vol, dims, dst, res, ws):
        check(lib().hdf_fill_holes(ptr(vol), int(label), int(connectivity), mode, *dims, ptr(dst), ptr(res), ptr(ws), ws.numel(),
                                   stream_ptr()), "hdf_fill_holes")
    return _run(volume, out, return_counts, _fill_workspaces, call)


def binary_dilation(volume, connectivity=6, iterations=1, label=0, border_value=0, out=None, return_counts=False):
    """the uint8 0 / 1 mask of the dilated mask, a device tensor shaped like `volume`.  Replaces
    scipy.ndimage.binary_dilation(mask, generate_binary_structure(3, c), iterations, border_value=border_value).
    out: a uint8 device tensor to write to -- `volume` itself for in place.  return_counts: also the device tensor int64
    [2] = voxels of the new mask, voxels that changed; nothing waits on the host unless the caller reads it."""
    return _morph(volume, DILATE, connectivity, iterations, label, border_value, MASK, out, return_counts)


def binary_erosion(volume, connectivity=6, iterations=1, label=0, border_value=0, out=None, return_counts=False):
    """scipy.ndimage.binary_erosion; arguments as binary_dilation"""
    return _morph(volume, ERODE, connectivity, iterations, label, border_value, MASK, out, return_counts)


def binary_opening(volume, connectivity=6, iterations=1, label=0, border_value=0, out=None, return_counts=False):
    """scipy.ndimage.binary_opening: `iterations` erosions, then as many dilations; arguments as binary_dilation"""
    return _morph(volume, OPEN, connectivity, iterations, label, border_value, MASK, out, return_counts)


def binary_closing(volume, connectivity=6, iterations=1, label=0, border_value=0, out=None, return_counts=False):
    """scipy.ndimage.binary_closing: `iterations` dilations, then as many erosions (with border_value = 0 an object that
    touches a face is eroded there, as in scipy); arguments as binary_dilation"""
    return _morph(volume, CLOSE, connectivity, iterations, label, border_value, MASK, out, return_counts)


def binary_fill_holes(volume, connectivity=6, label=0, out=None, return_counts=False):
    """the uint8 0 / 1 mask with its holes filled: the background components (under `connectivity`) that touch no face of
    the volume.  Replaces scipy.ndimage.binary_fill_holes(mask, generate_binary_structure(3, c))."""
    return _fill(volume, connectivity, label, MASK, out, return_counts)


def morph_class(volume, label, op, connectivity=6, iterations=1, border_value=0, out=None, return_counts=False):
    """the class map after `op` ('dilate' | 'erode' | 'open' | 'close') on class `label` (1..255): 0 where a voxel left the
    class, `label` where one joined it and held 0, the map's own value everywhere else -- another class is never
    overwritten, so cal_score / multi_* take the result"""
    if op not in OPS:
        raise ValueError(f"op must be one of {sorted(OPS)}, got {op!r}")
    return _morph(volume, OPS[op], connectivity, iterations, label, border_value, MAP, out, return_counts)


def fill_class_holes(volume, label, connectivity=6, out=None, return_counts=False):
    """the class map with the holes of class `label` (1..255) filled where they held 0; a voxel of another class inside a
    hole is kept"""
    return _fill(volume, connectivity, label, MAP, out, return_counts)
