"""Connected components of a label map on the device: what scipy.ndimage.label / find_objects / sum / maximum do on the
host after a copy of the map (117 MB for a 448x512x512 volume) and before a copy back.  The map that
sliding_window_predict returns goes through keep_largest_component or remove_small_components into cal_score / multi_*
without leaving the device.  Kernels: csrc/components.hip; definitions: include/hdf.h.  No CPU fallback.

connectivity is 6, 18 or 26 (scipy's generate_binary_structure(3, 1 | 2 | 3)); two voxels are adjacent only when they hold
the same non-zero value; label = 0 takes every non-zero value, label = k only the voxels equal to k.  Component ids are
1..n in ascending order of each component's smallest linear voxel index -- scipy's numbering.  A [H, W] input is the
depth-1 volume [1, H, W]: 6 / 18 / 26 are then the 4- / 8- / 8-neighbourhood."""
import struct

import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr, stream_ptr
from ._volume import WorkspaceCache, as_volume, check_out, clear_all

TABLE_COLS = ("size", "value", "first", "zmin", "zmax", "ymin", "ymax", "xmin", "xmax")
# one workspace per volume shape and stream (_volume.WorkspaceCache), about 5 bytes a voxel, in a cache of its own
_workspaces = WorkspaceCache("hdf_cc_workspace_bytes")


def clear_workspaces():
    """drop the cached workspaces: these, and those of the other entries on a volume (as hdf_rt.surface's)"""
    clear_all()


def _volume(a, what="volume"):
    """(uint8 [D][H][W] on the GPU, the caller's shape) from a device tensor or a numpy array, uint8 or bool, 3-D or 2-D"""
    return as_volume(a, what, dims=(2, 3), dtypes=(torch.uint8, torch.bool), who="connected components need")


def _label(vol, connectivity, label):
    """(ids int32 [D, H, W], result int64[2] = n, foreground voxels), both on the device"""
    shape = tuple(int(s) for s in vol.shape)
    with torch.cuda.device(vol.device):
        ws = _workspaces.workspace(vol.device, *shape)
        ids = torch.empty(shape, dtype=torch.int32, device=vol.device)
        res = torch.empty(2, dtype=torch.int64, device=vol.device)
        check(lib().hdf_cc_label(ptr(vol), int(label), int(connectivity), *shape, ptr(ids), ptr(res), ptr(ws), ws.numel(),
                                 stream_ptr()), "hdf_cc_label")
    return ids, res


def connected_components(volume, connectivity=26, label=0):
    """(ids, count): ids an int32 device tensor shaped like `volume`, count a 0-dim device tensor -- nothing waits on the
    host unless the caller reads it.  Replaces scipy.ndimage.label(volume == k, generate_binary_structure(3, c))."""
    vol, shape = _volume(volume)
    ids, res = _label(vol, connectivity, label)
    return ids.view(shape), res[0]


def component_table(volume, ids, score=None, capacity=4096):
    """the device table int64 [capacity, 9] (TABLE_COLS; row id-1; rows past the number of components are zeros,
    components past `capacity` are left out), and score_max fp32 [capacity] when a non-negative fp32 `score` volume is
    given (the lesion's confidence when score is a class probability).  Replaces find_objects / sum / maximum."""
    vol, _ = _volume(volume)
    shape = tuple(int(s) for s in vol.shape)
    if not (torch.is_tensor(ids) and ids.dtype == torch.int32 and ids.device == vol.device and ids.numel() == vol.numel()):
        raise ValueError("ids must be the int32 device tensor connected_components returned for this volume")
    ids = ids.contiguous()
    capacity = int(capacity)
    with torch.cuda.device(vol.device):
        table = torch.empty((max(capacity, 0), 9), dtype=torch.int64, device=vol.device)
        smax = None
        if score is not None:
            if not torch.is_tensor(score):
                score = torch.from_numpy(np.ascontiguousarray(score))
            if score.numel() != vol.numel():
                raise ValueError(f"score {tuple(score.shape)} does not match the volume {shape}")
            score = score.to(vol.device, torch.float32).contiguous()
            smax = torch.empty(max(capacity, 0), dtype=torch.float32, device=vol.device)
        check(lib().hdf_cc_table(ptr(vol), ptr(ids), ptr(score), *shape, capacity, ptr(table), ptr(smax), stream_ptr()),
              "hdf_cc_table")
    return table if score is None else (table, smax)


def component_stats(volume, connectivity=26, label=0, score=None, capacity=4096):
    """label, table, ONE copy to the host: a list with a dict per component, in id order -- size, value, first (linear
    voxel index), bbox = (zmin, zmax, ymin, ymax, xmin, xmax) with inclusive maxima, score_max (None without a score).
    More than `capacity` components is an error."""
    vol, _ = _volume(volume)
    ids, res = _label(vol, connectivity, label)
    out = component_table(vol, ids, score, capacity)
    table, smax = (out, None) if score is None else out
    parts = [res, table.reshape(-1)]
    if smax is not None:
        parts.append(smax.view(torch.int32).to(torch.int64))
    host = torch.cat(parts).cpu().tolist()          # the one D2H copy
    n, cap = host[0], table.shape[0]
    if n > cap:
        raise _lib.HdfError(f"component_stats: {n} components, capacity {cap}")
    stats = []
    for i in range(n):
        r = host[2 + 9 * i: 11 + 9 * i]
        sm = None if smax is None else struct.unpack("<f", struct.pack("<i", host[2 + 9 * cap + i]))[0]
        stats.append({"size": r[0], "value": r[1], "first": r[2], "bbox": tuple(r[3:9]), "score_max": sm})
    return stats


def _filter(volume, connectivity, label, min_size, keep_largest, out):
    vol, shape = _volume(volume)
    dims = tuple(int(s) for s in vol.shape)
    ids, _ = _label(vol, connectivity, label)
    dst = check_out(out, vol, shape)
    with torch.cuda.device(vol.device):
        ws = _workspaces.workspace(vol.device, *dims)
        res = torch.empty(2, dtype=torch.int64, device=vol.device)
        check(lib().hdf_cc_filter(ptr(vol), ptr(ids), *dims, int(min_size), int(keep_largest), ptr(dst), ptr(res), ptr(ws),
                                  ws.numel(), stream_ptr()), "hdf_cc_filter")
    return dst.view(shape)


def keep_largest_component(volume, connectivity=26, label=0, min_size=0, out=None):
    """the uint8 map with, of every value (label = 0) or of value `label` alone, only its largest component (a tie: the
    one whose first voxel comes first) and only if that has at least min_size voxels; everything else 0.  out: a uint8
    device tensor to write to -- `volume` itself for in place."""
    return _filter(volume, connectivity, label, min_size, 1, out)


def remove_small_components(volume, min_size, connectivity=26, label=0, out=None):
    """the uint8 map without the components of fewer than min_size voxels (with label = k the other values go too)"""
    return _filter(volume, connectivity, label, min_size, 0, out)
