"""Measurements of an image under an id map on the device: what scipy.ndimage's sum_labels, mean, variance /
standard_deviation, minimum / maximum, minimum_position / maximum_position and center_of_mass do on the host, one call per
statistic and channel, after a copy of the int32 id map and of every image channel (470 MB each for a 448x512x512 volume).
The ids of connected_components, the index map of extract_lesion_candidates or a class map go in with the image the model
saw; per lesion come out MTV, SUVmax, SUVmean and TLG (pet_lesion_measures), or volume, centroid and the mean probability
as a confidence (region_stats).  Kernels: csrc/measure.hip; definitions and the numerical contract: include/hdf.h.  No CPU
fallback.

Rank statistics -- what scipy.ndimage.median and np.percentile per id, channel and level do on the host after a full sort of
every component -- come from region_quantiles (device tensors), region_order_stats (one dict per id) and region_median:
the 10th and 90th percentile, the IQR, the median SUV or ADC of a lesion.  Kernels: csrc/quantiles.hip, an exact radix
select; entry hdf_cc_quantiles.

ids: any integer numbering, a value below 0 counting as 0; image: [D, H, W] (one channel) or [C, D, H, W], C up to 8.  2-D
inputs ([H, W] with [H, W] or [C, H, W]) are the depth-1 volume.  On a tie the position of an extremum is the smallest linear
index -- np.argmin / np.argmax, not scipy's maximum_position, which returns the last one."""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr, stream_ptr
from ._volume import WorkspaceCache

STAT_COLS = ("sum", "mean", "m2", "min", "max", "wz", "wy", "wx")
# one workspace per (channels, capacity) and stream, 24 + 272 C bytes an id
_workspaces = WorkspaceCache("hdf_cc_measure_workspace_bytes")
# one per (channels, capacity, levels) and stream, 56 bytes an id
_quantile_workspaces = WorkspaceCache("hdf_cc_quantiles_workspace_bytes")


def _inputs(ids, image):
    """(ids int32 [D][H][W], image fp32 [C][D][H][W], both contiguous on the GPU)"""
    if not torch.cuda.is_available():
        raise _lib.HdfError("region measurements need a GPU (there is no CPU path)")
    if not torch.is_tensor(ids):
        ids = torch.from_numpy(np.ascontiguousarray(ids))
    if not torch.is_tensor(image):
        image = torch.from_numpy(np.ascontiguousarray(image))
    if ids.dim() not in (2, 3) or ids.is_floating_point() or ids.is_complex():
        raise ValueError(f"ids must be an integer map [D, H, W] or [H, W], got {ids.dtype} {tuple(ids.shape)}")
    if image.dim() == ids.dim():
        image = image[None]
    if image.dim() != ids.dim() + 1 or tuple(image.shape[1:]) != tuple(ids.shape):
        raise ValueError(f"image {tuple(image.shape)} does not match the ids {tuple(ids.shape)}: the same shape, or [C, ...]")
    if not image.is_floating_point():
        raise ValueError(f"image must be a floating-point tensor, got {image.dtype}")
    dev = ids.device if ids.is_cuda else (image.device if image.is_cuda else torch.device("cuda"))
    ids = ids.to(dev, torch.int32).contiguous()
    image = image.to(dev, torch.float32).contiguous()
    if ids.dim() == 2:
        ids, image = ids[None], image[:, None]
    return ids, image


def region_measure(ids, image, capacity=4096):
    """(geom int64 [capacity, 4], stats fp64 [C, capacity, 8], pos int64 [C, capacity, 2], result int64 [4]) on the device;
    nothing waits on the host.  Row id-1: geom = n, sum z, sum y, sum x; stats (STAT_COLS) = sum, mean, M2 = sum (x - mean)^2,
    min, max and the three coordinate sums weighted by x; pos = the linear index of the minimum and of the maximum; result =
    the largest id met, the voxels with id > 0, those with id in 1..capacity, 0.  Ids above capacity are left out; a row no
    voxel holds is zeros."""
    ids, image = _inputs(ids, image)
    C, (D, H, W) = int(image.shape[0]), (int(s) for s in ids.shape)
    capacity = int(capacity)
    rows = max(capacity, 0)
    with torch.cuda.device(ids.device):
        ws = _workspaces.workspace(ids.device, C, capacity)
        geom = torch.empty((rows, 4), dtype=torch.int64, device=ids.device)
        stats = torch.empty((C, rows, 8), dtype=torch.float64, device=ids.device)
        pos = torch.empty((C, rows, 2), dtype=torch.int64, device=ids.device)
        res = torch.empty(4, dtype=torch.int64, device=ids.device)
        check(lib().hdf_cc_measure(ptr(ids), ptr(image), C, D, H, W, capacity, ptr(geom), ptr(stats), ptr(pos), ptr(res), ptr(ws),
                                   ws.numel(), stream_ptr()), "hdf_cc_measure")
    return geom, stats, pos, res


def _div(a, b):
    """a / b as numpy divides: nan for 0 / 0, an infinity for x / 0 (scipy's center_of_mass of a component that sums to 0)"""
    if b != 0.0:
        return a / b
    return math.nan if a == 0.0 or a != a else math.copysign(math.inf, a) * math.copysign(1.0, b)


def _zyx(index, H, W):
    return (index // (H * W), index // W % H, index % W)


def _ndim(a):
    return a.dim() if torch.is_tensor(a) else np.ndim(a)


def stats_from_host(geom, stats, pos, shape, spacing=None):
    """the list of region_stats from host arrays shaped like region_measure's outputs; shape: (D, H, W)"""
    _, H, W = shape
    geom, stats, pos = np.asarray(geom), np.asarray(stats), np.asarray(pos)
    sp = None if spacing is None else tuple(float(s) for s in spacing)
    if sp is not None and (len(sp) != 3 or not all(s > 0.0 and math.isfinite(s) for s in sp)):
        raise ValueError(f"spacing must be three positive finite numbers (z, y, x), got {spacing}")
    out = []
    for row in np.flatnonzero(geom[:, 0] > 0).tolist():
        n, sz, sy, sx = (int(v) for v in geom[row])
        d = {"id": row + 1, "size": n, "centroid": (sz / n, sy / n, sx / n), "channels": []}
        if sp is not None:
            d["volume_mm3"] = n * sp[0] * sp[1] * sp[2]
            d["centroid_mm"] = tuple(c * s for c, s in zip(d["centroid"], sp))
        for c in range(stats.shape[0]):
            s1, mean, m2, lo, hi, wz, wy, wx = (float(v) for v in stats[c, row])
            com = (_div(wz, s1), _div(wy, s1), _div(wx, s1))
            ch = {"sum": s1, "mean": mean, "variance": m2 / n, "std": math.sqrt(m2 / n) if m2 >= 0.0 else math.nan,
                  "min": lo, "max": hi,
                  "argmin": _zyx(int(pos[c, row, 0]), H, W), "argmax": _zyx(int(pos[c, row, 1]), H, W),
                  "center_of_mass": com}
            if sp is not None:
                ch["center_of_mass_mm"] = tuple(a * s for a, s in zip(com, sp))
            d["channels"].append(ch)
        out.append(d)
    return out


def _measure_to_host(ids, image, capacity, who):
    geom, stats, pos, res = region_measure(ids, image, capacity)
    C, cap = int(stats.shape[0]), int(geom.shape[0])
    # ONE copy: the fp64 rows travel as their bits
    host = torch.cat([res, geom.reshape(-1), stats.view(torch.int64).reshape(-1), pos.reshape(-1)]).cpu().numpy()
    if int(host[0]) > cap:
        raise _lib.HdfError(f"{who}: ids up to {int(host[0])}, capacity {cap}")
    g = host[4: 4 + 4 * cap].reshape(cap, 4)
    s = host[4 + 4 * cap: 4 + 4 * cap + 8 * C * cap].view(np.float64).reshape(C, cap, 8)
    p = host[4 + 4 * cap + 8 * C * cap:].reshape(C, cap, 2)
    return g, s, p


def _shape3(ids):
    shape = tuple(int(s) for s in ids.shape)
    return shape if len(shape) == 3 else (1,) + shape


def region_stats(ids, image, capacity=4096, spacing=None):
    """measure, ONE copy to the host: a list with a dict per id that is present, in id order -- id, size, centroid (z, y, x;
    geometric, from the exact integer sums) and channels, a list with a dict per channel: sum, mean, variance (M2 / n,
    scipy's), std, min, max, argmin and argmax as (z, y, x), center_of_mass (W / S1: nan or inf where scipy gives them).
    With spacing = (sz, sy, sx) in mm: volume_mm3, centroid_mm and per channel center_of_mass_mm.  For a 2-D input the z of
    every triple is 0.  An id above `capacity` is an HdfError."""
    g, s, p = _measure_to_host(ids, image, capacity, "region_stats")
    return stats_from_host(g, s, p, _shape3(ids), spacing)


def pet_lesion_measures(ids, suv, spacing, capacity=4096):
    """per lesion of `ids` (in id order) the PET measures of the HECKTOR workload from the SUV volume [D, H, W]: a list of
    dicts id, size, MTV (the metabolic tumour volume in ml = voxels x voxel volume in mm3 / 1000), SUVmax, SUVmean, TLG =
    SUVmean x MTV, and SUVpeak_at, the (z, y, x) of SUVmax.  Host arithmetic on the one copy of region_stats."""
    if _ndim(suv) != _ndim(ids):
        raise ValueError("suv must be one channel, shaped like ids")
    out = []
    for d in region_stats(ids, suv, capacity, spacing):
        ch = d["channels"][0]
        mtv = d["volume_mm3"] / 1000.0
        out.append({"id": d["id"], "size": d["size"], "MTV": mtv, "SUVmax": ch["max"], "SUVmean": ch["mean"],
                    "TLG": ch["mean"] * mtv, "SUVpeak_at": ch["argmax"]})
    return out


def _device_inputs(ids, image):
    """_inputs for the order statistics, which take device tensors only: they exist to spare the copies, so a host array
    is a mistake of the caller's, not something to upload quietly"""
    for name, a in (("ids", ids), ("image", image)):
        if not (torch.is_tensor(a) and a.is_cuda):
            raise ValueError(f"{name} must be a tensor on the GPU, got {type(a).__name__}"
                             + (f" on {a.device}" if torch.is_tensor(a) else ""))
    if ids.device != image.device:
        raise ValueError(f"ids on {ids.device}, image on {image.device}")
    return _inputs(ids, image)


def _levels(q):
    levels = [float(v) for v in (q if isinstance(q, (tuple, list, np.ndarray)) else (q,))]
    return levels, (ctypes.c_double * max(len(levels), 1))(*levels)


def region_quantiles(ids, image, q=(0.5,), capacity=4096):
    """(count int64 [capacity], values fp64 [C, capacity, Q, 3], result int64 [4]) on the device; nothing waits on the host.
    q: levels in [0, 1], in any order (0.5 the median, 0 the minimum, 1 the maximum).  Row id-1: count = n; values, per
    channel and level = s_lo, s_hi and s_lo + frac (s_hi - s_lo), with s the sorted values of the id, h = q (n - 1),
    lo = floor(h), frac = h - lo and hi = lo + (frac > 0): np.quantile's default, the linear interpolation.  result as
    region_measure's.  Ids above capacity are left out; a row no voxel holds is zeros.  Exact order statistics: every output is
    the same in every bit from call to call.  ids and image must be device tensors, otherwise shaped as region_measure
    takes them."""
    ids, image = _device_inputs(ids, image)
    Cn, (D, H, W) = int(image.shape[0]), (int(s) for s in ids.shape)
    capacity = int(capacity)
    rows = max(capacity, 0)
    levels, host_q = _levels(q)
    Q = len(levels)
    with torch.cuda.device(ids.device):
        ws = _quantile_workspaces.workspace(ids.device, Cn, capacity, Q)
        count = torch.empty((rows,), dtype=torch.int64, device=ids.device)
        values = torch.empty((Cn, rows, Q, 3), dtype=torch.float64, device=ids.device)
        res = torch.empty(4, dtype=torch.int64, device=ids.device)
        check(lib().hdf_cc_quantiles(ptr(ids), ptr(image), Cn, D, H, W, capacity, host_q, Q, ptr(count), ptr(values), ptr(res),
                                     ptr(ws), ws.numel(), stream_ptr()), "hdf_cc_quantiles")
    return count, values, res


def region_order_stats(ids, image, q=(0.1, 0.5, 0.9), capacity=4096):
    """quantiles, ONE copy to the host: a list with a dict per id that is present, in id order -- id, size and channels, a
    list with a dict per channel: quantiles (the interpolated values in the order of q), lower and upper (the order
    statistics s_lo and s_hi they were formed from).  An id above `capacity` is an HdfError."""
    count, values, res = region_quantiles(ids, image, q, capacity)
    Cn, cap, Q = (int(s) for s in values.shape[:3])
    host = torch.cat([res, count, values.view(torch.int64).reshape(-1)]).cpu().numpy()
    if int(host[0]) > cap:
        raise _lib.HdfError(f"region_order_stats: ids up to {int(host[0])}, capacity {cap}")
    n = host[4: 4 + cap]
    v = host[4 + cap:].view(np.float64).reshape(Cn, cap, Q, 3)
    return [{"id": row + 1, "size": int(n[row]),
             "channels": [{"quantiles": v[c, row, :, 2].tolist(), "lower": v[c, row, :, 0].tolist(),
                           "upper": v[c, row, :, 1].tolist()} for c in range(Cn)]}
            for row in np.flatnonzero(n > 0).tolist()]


def region_median(ids, image, capacity=4096):
    """fp64 [C, capacity] on the device: the median of every id in every channel (the mean of the two middle values where
    the id has an even number of voxels), 0 for an id no voxel holds"""
    return region_quantiles(ids, image, (0.5,), capacity)[1][:, :, 0, 2]
