"""The average-surface-distance definitions of include/hdf.h restated in integers (no GPU part), and the planted defects
the GPU tests' inputs must be able to see.  Inputs, the squared distance map and the bin count are tests/surface_ref.py's.

T = (target == label), P = (prediction == label) over one uint8 volume [D][H][W], unit spacing.  E6(M): the voxels of M
with a face neighbour not in M, a neighbour outside the volume counting as not in M -- written here with shifted copies
of the zero-padded mask, not with scipy's erosion (the test against MONAI's call sequence uses that).  Everything up to
the histograms is an exact integer; the two sums are math.fsum over hist[k] sqrt(k), and `floats` forms the three
numbers in fp64 the way hdf_rt.surface.asd_from_result does."""
import functools
import math

import numpy as np
from scipy import ndimage as ndi

import surface_ref as sr

IN_T, IN_P, E6_T, E6_P = 1, 2, 64, 128
DEFECTS = ("c6_edges", "erode26", "to_mask", "mean_of_means", "rms", "directed")


def edges(mask):
    """E6(mask)"""
    m = np.pad(mask, 1)
    inner = (m[:-2, 1:-1, 1:-1] & m[2:, 1:-1, 1:-1] & m[1:-1, :-2, 1:-1] & m[1:-1, 2:, 1:-1] & m[1:-1, 1:-1, :-2]
             & m[1:-1, 1:-1, 2:])
    return mask & ~inner


def _edges(mask, defect):
    if defect == "c6_edges":                      # in-volume neighbours only: the rule of hdf_op_mask_flags
        return sr.border(mask, sr.S6)
    if defect == "erode26":
        return mask & ~ndi.binary_erosion(mask, structure=sr.S26, border_value=0)
    return edges(mask)


def fsum_sqrt(hist):
    k = np.nonzero(hist)[0]
    return math.fsum(int(hist[i]) * math.sqrt(int(i)) for i in k)


def floats(n_t, n_p, sum_a, sum_b):
    """ASD (pooled over both directions), prediction -> ground truth, ground truth -> prediction"""
    nan, inf = float("nan"), float("inf")

    def directed(total, n_from, n_to):
        return nan if n_from == 0 else inf if n_to == 0 else total / n_from

    sym = (nan if n_t == n_p else inf) if n_t == 0 or n_p == 0 else (sum_a + sum_b) / (n_p + n_t)
    return {"ASD": sym, "ASD_pred_to_gt": directed(sum_a, n_p, n_t), "ASD_gt_to_pred": directed(sum_b, n_t, n_p)}


def asd(target, prediction, label, defect=None):
    """dict: flags uint8, counts [|E6(T)|, |E6(P)|], d2ET / d2EP int64, histA / histB int64[hist_bins], sumA / sumB
    float, scores.  defect: one of DEFECTS, a deliberately wrong reading of the definitions (tests/test_asd_ref_cpu.py)."""
    assert defect is None or defect in DEFECTS
    T, P = target == label, prediction == label
    eT, eP = _edges(T, defect), _edges(P, defect)
    flags = (T * IN_T + P * IN_P + eT * E6_T + eP * E6_P).astype(np.uint8)
    counts = [int(eT.sum()), int(eP.sum())]
    d2ET, d2EP = sr.d2_of(T if defect == "to_mask" else eT), sr.d2_of(P if defect == "to_mask" else eP)
    nb = sr.hist_bins(T.shape)
    hA, hB = np.zeros(nb, np.int64), np.zeros(nb, np.int64)
    if counts[0] and counts[1]:                   # otherwise one map holds the no-seed sentinel: there are no distances
        hA = np.bincount(d2ET[eP], minlength=nb).astype(np.int64)
        hB = np.bincount(d2EP[eT], minlength=nb).astype(np.int64)
    sA, sB = fsum_sqrt(hA), fsum_sqrt(hB)
    out = floats(counts[0], counts[1], sA, sB)
    if counts[0] and counts[1]:
        if defect == "mean_of_means":
            out["ASD"] = (sA / counts[1] + sB / counts[0]) / 2
        elif defect == "rms":
            k = np.arange(nb)
            out["ASD"] = math.sqrt(int(((hA + hB) * k).sum()) / (counts[0] + counts[1]))
        elif defect == "directed":
            out["ASD"] = out["ASD_pred_to_gt"]
    return dict(flags=flags, counts=counts, d2ET=d2ET, d2EP=d2EP, histA=hA, histB=hB, sumA=sA, sumB=sB, scores=out)


@functools.lru_cache(maxsize=None)
def case_ref(shape, kind):
    """asd() of surface_ref.case(shape, kind); shared: do not write to its arrays"""
    t, p, k = sr.case(shape, kind)
    return asd(t, p, k)


def same_float(a, b, rel):
    """NaN and inf only in the same places, everything else within rel"""
    if math.isnan(a) or math.isnan(b):
        return math.isnan(a) and math.isnan(b)
    if math.isinf(a) or math.isinf(b):
        return a == b
    return abs(a - b) <= rel * abs(b)
