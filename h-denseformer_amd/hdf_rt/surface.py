"""Scoring a label map against the ground truth on the device (reference: cal_score, multi_dice, multi_hd, multi_vs,
multi_jc, metrics.py:156-309).  The reference makes one SimpleITK pass per class on the host -- overlap measures, two
signed Maurer distance maps, two label contours, a percentile over the surface distances.  Here a class is one
hdf_surface_distances call (mask flags, two exact squared distance transforms, a histogram, a select: csrc/surface.hip)
that leaves twelve integers on the device; all classes are enqueued, the rows come back in ONE copy and the floats are
formed in fp64 on the host.  Definitions: include/hdf.h.  No CPU fallback.

The average surface distance (reference: cal_asd, multi_asd, utils.py:165-191, MONAI's SurfaceDistanceMetric on the host)
is a call of its own, hdf_surface_asd (csrc/surface_asd.hip): MONAI's edge set and its distance to the other EDGE SET are
not the contour and the Maurer map of cal_score.  It leaves four integers per class; the rest is the same.

Physical units: every wrapper takes `spacing=None`.  None is the path above, unchanged (distances in voxels).  A triple
(sz, sy, sx) -- the voxel size along the axes of the array AS IT IS PASSED, [D, H, W] -- takes hdf_surface_distances_mm /
hdf_surface_asd_mm (csrc/surface_mm.hip): the same flags, seed sets and contours, fp64 squared distances weighted per axis,
an exact select over their bit patterns in place of the histogram.  The rest is the same again."""
import ctypes
import math
import struct

import numpy as np
import torch

from ._lib import check, lib, ptr, stream_ptr
from ._volume import WorkspaceCache, as_volume, clear_all

KEYS = ("Jaccard", "Dice", "VolumeSimilarity", "HausdorffDistance", "HausdorffDistance95")
# one workspace per volume shape and stream (_volume.WorkspaceCache): about 9 bytes a voxel plus the histogram
_workspaces = WorkspaceCache("hdf_surface_workspace_bytes")
# the same for hdf_surface_asd, which needs one histogram more: a cache of its own, so that neither call is ever handed
# the other's allocation
_asd_workspaces = WorkspaceCache("hdf_surface_asd_workspace_bytes")
# and for the entries that take a spacing (fp64 maps: about 17 bytes a voxel), shared by the two of them
_mm_workspaces = WorkspaceCache("hdf_surface_mm_workspace_bytes")
ASD_KEYS = ("ASD", "ASD_pred_to_gt", "ASD_gt_to_pred")


def clear_workspaces():
    """drop the cached workspaces (a caller that is done scoring, or moves on to another volume shape): these, and those
    of the connected-component, morphology and overlap-table entries"""
    clear_all()


def _volume(a, what):
    """uint8 [D][H][W] on the GPU from a device tensor or a numpy array of any dtype (uploaded once)"""
    return as_volume(a, what, dims=(3,), who="surface metrics need")[0]


def _spacing(spacing):
    """(sz, sy, sx) as the host array of three doubles the C entries read; the entries themselves refuse a bad value"""
    s = [float(v) for v in spacing]
    if len(s) != 3:
        raise ValueError(f"spacing must be (sz, sy, sx), got {spacing!r}")
    return (ctypes.c_double * 3)(*s)


def _f64(bits):
    return struct.unpack("<d", struct.pack("<Q", int(bits) & 0xFFFFFFFFFFFFFFFF))[0]


def scores_from_result_mm(row):
    """the five numbers of cal_score in fp64 from one result[12] row of hdf_surface_distances_mm: words 5, 7 and 8 are the
    bit patterns of squared physical distances"""
    nT, nP, nI, _c6t, _c6p, hd2, _n, slo, shi, _lo, r, valid = (int(v) for v in row)
    return _scores(nT, nP, nI, _f64(hd2), _f64(slo), _f64(shi), r, valid)


def scores_from_result(row):
    """the five numbers of cal_score in fp64 from one result[12] row of hdf_surface_distances"""
    nT, nP, nI, _c6t, _c6p, hd2, _n, slo, shi, _lo, r, valid = (int(v) for v in row)
    return _scores(nT, nP, nI, hd2, slo, shi, r, valid)


def _scores(nT, nP, nI, hd2, slo, shi, r, valid):
    nan = float("nan")
    out = {"Jaccard": nI / (nT + nP - nI) if nT + nP - nI else nan,
           "Dice": 2 * nI / (nT + nP) if nT + nP else nan,
           "VolumeSimilarity": 2 * (nT - nP) / (nT + nP) if nT + nP else nan,   # Execute(target, predict): target is ITK's source
           "HausdorffDistance": nan, "HausdorffDistance95": nan}
    if valid:
        a, b = math.sqrt(slo), math.sqrt(shi)
        out["HausdorffDistance"] = math.sqrt(hd2)
        out["HausdorffDistance95"] = a + (b - a) * r / 100    # np.percentile(., 95), linear
    return out


def _pair(target, prediction):
    """both volumes on the target's device, and their common shape"""
    tgt, prd = _volume(target, "target"), _volume(prediction, "prediction")
    if prd.device != tgt.device:
        prd = prd.to(tgt.device)
    if tgt.shape != prd.shape:
        raise ValueError(f"target {tuple(tgt.shape)} and prediction {tuple(prd.shape)} differ")
    return tgt, prd, tuple(int(s) for s in tgt.shape)


def surface_scores(target, prediction, labels, spacing=None):
    """one dict of KEYS per label in `labels` (each 1..255), for two uint8 volumes [D, H, W].  spacing: None (distances
    in voxels) or the voxel size (sz, sy, sx) along the array's axes (HausdorffDistance and HausdorffDistance95 in its
    unit, both directions)"""
    tgt, prd, shape = _pair(target, prediction)
    labels = [int(k) for k in labels]
    if spacing is not None:
        sp = _spacing(spacing)
        with torch.cuda.device(tgt.device):
            ws = _mm_workspaces.workspace(tgt.device, *shape)
            rows = torch.empty((max(len(labels), 1), 12), dtype=torch.int64, device=tgt.device)
            for i, k in enumerate(labels):
                check(lib().hdf_surface_distances_mm(ptr(tgt), ptr(prd), k, *shape, sp, ptr(ws), ws.numel(), ptr(rows[i]),
                                                     stream_ptr()), "hdf_surface_distances_mm")
            host = rows.cpu()          # the one D2H copy, after every class is enqueued
        return [scores_from_result_mm(host[i].tolist()) for i in range(len(labels))]
    with torch.cuda.device(tgt.device):
        ws = _workspaces.workspace(tgt.device, *shape)
        rows = torch.empty((max(len(labels), 1), 12), dtype=torch.int64, device=tgt.device)
        for i, k in enumerate(labels):
            check(lib().hdf_surface_distances(ptr(tgt), ptr(prd), k, *shape, ptr(ws), ws.numel(), ptr(rows[i]), None, 0,
                                              stream_ptr()), "hdf_surface_distances")
        host = rows.cpu()          # the one D2H copy, after every class is enqueued
    return [scores_from_result(host[i].tolist()) for i in range(len(labels))]


def cal_score(predict, target, spacing=None):
    """metrics.cal_score(predict, target) for two boolean or uint8 masks (non-zero = inside): a dict of KEYS.  The
    reference's FalseNegativeError / FalsePositiveError are left out (none of its wrappers reads them).  spacing: as
    surface_scores -- what the reference gets from the SimpleITK images it is handed (useImageSpacing=True)."""
    prd, tgt = _volume(predict, "predict"), _volume(target, "target")
    return surface_scores((tgt != 0).to(torch.uint8), (prd != 0).to(torch.uint8), [1], spacing)[0]


def _multi(key, y_true, y_pred, num_classes, spacing=None):
    vals = [round(s[key], 4) for s in surface_scores(y_true, y_pred, range(1, num_classes + 1), spacing)]
    return vals, round(np.mean(vals), 4)


def multi_dice(y_true, y_pred, num_classes, spacing=None):
    """(spacing does not enter an overlap measure; it selects the call that computes them all)"""
    return _multi("Dice", y_true, y_pred, num_classes, spacing)


def multi_hd(y_true, y_pred, num_classes, spacing=None):
    """per-class HausdorffDistance95, like the reference's multi_hd; in the unit of `spacing` = (sz, sy, sx) when given"""
    return _multi("HausdorffDistance95", y_true, y_pred, num_classes, spacing)


def multi_vs(y_true, y_pred, num_classes, spacing=None):
    """(spacing: as multi_dice)"""
    return _multi("VolumeSimilarity", y_true, y_pred, num_classes, spacing)


def multi_jc(y_true, y_pred, num_classes, spacing=None):
    """(spacing: as multi_dice)"""
    return _multi("Jaccard", y_true, y_pred, num_classes, spacing)


# ------------------------------------------------------------------------------------------- average surface distance
def asd_from_result(row):
    """the symmetric and the two directed average surface distances in fp64 from one result[4] row of hdf_surface_asd
    (|E6(T)|, |E6(P)| and the bit patterns of the two sums).  Empty edge sets as MONAI's get_surface_distance treats them:
    nothing to measure from is NaN, nothing to measure to is +inf."""
    n_t, n_p, bits_a, bits_b = (int(v) for v in row)
    sum_a, sum_b = (struct.unpack("<d", struct.pack("<Q", b & 0xFFFFFFFFFFFFFFFF))[0] for b in (bits_a, bits_b))
    nan, inf = float("nan"), float("inf")

    def directed(total, n_from, n_to):
        return nan if n_from == 0 else inf if n_to == 0 else total / n_from

    if n_t == 0 or n_p == 0:
        sym = nan if n_t == n_p else inf
    else:
        sym = (sum_a + sum_b) / (n_p + n_t)         # the pooled mean, not the mean of the two means
    return {"ASD": sym, "ASD_pred_to_gt": directed(sum_a, n_p, n_t), "ASD_gt_to_pred": directed(sum_b, n_t, n_p)}


def asd_scores(target, prediction, labels, spacing=None):
    """one dict of ASD_KEYS per label in `labels` (each 1..255), for two uint8 volumes [D, H, W].  spacing: None
    (distances in voxels) or the voxel size (sz, sy, sx) along the axes of the arrays as they are passed"""
    tgt, prd, shape = _pair(target, prediction)
    labels = [int(k) for k in labels]
    if spacing is not None:
        sp = _spacing(spacing)
        with torch.cuda.device(tgt.device):
            ws = _mm_workspaces.workspace(tgt.device, *shape)
            rows = torch.empty((max(len(labels), 1), 4), dtype=torch.int64, device=tgt.device)
            for i, k in enumerate(labels):
                check(lib().hdf_surface_asd_mm(ptr(tgt), ptr(prd), k, *shape, sp, ptr(ws), ws.numel(), ptr(rows[i]),
                                               stream_ptr()), "hdf_surface_asd_mm")
            host = rows.cpu()          # the one D2H copy, after every class is enqueued
        return [asd_from_result(host[i].tolist()) for i in range(len(labels))]
    with torch.cuda.device(tgt.device):
        ws = _asd_workspaces.workspace(tgt.device, *shape)
        rows = torch.empty((max(len(labels), 1), 4), dtype=torch.int64, device=tgt.device)
        for i, k in enumerate(labels):
            check(lib().hdf_surface_asd(ptr(tgt), ptr(prd), k, *shape, ptr(ws), ws.numel(), ptr(rows[i]), None, 0,
                                        stream_ptr()), "hdf_surface_asd")
        host = rows.cpu()          # the one D2H copy, after every class is enqueued
    return [asd_from_result(host[i].tolist()) for i in range(len(labels))]


def _mask(a, what):
    """a boolean or uint8 mask as [D, H, W], or in the reference's [1, 1, a, b, c] form (utils.py:180): 0 / 1 uint8"""
    if not torch.is_tensor(a):
        a = torch.from_numpy(np.ascontiguousarray(a))
    if a.dim() == 5 and a.shape[0] == 1 and a.shape[1] == 1:
        a = a[0, 0]
    return (_volume(a, what) != 0).to(torch.uint8)


def cal_asd(predict, target, spacing=None):
    """utils.cal_asd(predict, target) for one pair of boolean or uint8 masks (non-zero = inside), [D, H, W] or the
    reference's [1, 1, a, b, c], numpy or torch, host or device: MONAI's symmetric average surface distance as a float.
    spacing: None, or (sz, sy, sx) along the three volume axes of the masks as they are passed (what MONAI hands to
    scipy's distance_transform_edt(sampling=...))"""
    prd, tgt = _mask(predict, "predict"), _mask(target, "target")
    return asd_scores(tgt, prd, [1], spacing)[0]["ASD"]


def multi_asd(y_true, y_pred, num_classes, spacing=None):
    """utils.multi_asd(y_true, y_pred, num_classes) for two label maps [D, H, W]: (per-class ASD rounded to 4 places,
    their mean rounded likewise); an inf or a NaN goes through np.mean as it does in the reference.  The reference's
    permute(1, 2, 0) only renames the axes (unit spacing): the maps are taken as they are.  With a spacing that renaming
    matters: the reference permutes the axes BEFORE MONAI sees them, so a spacing given there is in the permuted order.
    Here `spacing` = (sz, sy, sx) follows the axes of the arrays the caller passes, [D, H, W], and nothing is permuted."""
    vals = [round(s["ASD"], 4) for s in asd_scores(y_true, y_pred, range(1, num_classes + 1), spacing)]
    return vals, round(np.mean(vals), 4)
