"""The surface-distance definitions of include/hdf.h restated with scipy (no GPU part), the inputs of the GPU tests and
the planted defects those inputs must be able to see.

T = (target == label), P = (prediction == label) over one uint8 volume [D][H][W], unit spacing.  Neighbours outside the
volume do not exist (binary_erosion with border_value=1).  Everything up to `result` is an exact integer; `scores` forms
the floats in fp64 the way hdf_rt.surface does."""
import functools
import math

import numpy as np
from scipy import ndimage as ndi

NO_SEED = 0x3FFFFFFF
IN_T, IN_P, B26_T, B26_P, C6_T, C6_P = 1, 2, 4, 8, 16, 32
S26 = np.ones((3, 3, 3), bool)
S6 = ndi.generate_binary_structure(3, 1)
DEFECTS = ("border6", "edge_background", "nearest_rank", "hd_on_contours")


def border(mask, structure, edge_background=False):
    """voxels of mask with an in-volume neighbour (per structure) outside mask"""
    return mask & ~ndi.binary_erosion(mask, structure=structure, border_value=0 if edge_background else 1)


def d2_of(seed):
    """int64 squared distance of every voxel to the nearest True voxel of seed; NO_SEED everywhere when there is none"""
    if not seed.any():
        return np.full(seed.shape, NO_SEED, np.int64)
    idx = ndi.distance_transform_edt(~seed, return_distances=False, return_indices=True)
    grid = np.indices(seed.shape)
    return ((idx.astype(np.int64) - grid) ** 2).sum(0)


def hist_bins(shape):
    return int(sum((s - 1) ** 2 for s in shape)) + 1


def select(n):
    """(lo, r, hi) of the linear 95th percentile over n sorted values"""
    q = 95 * (n - 1)
    lo, r = divmod(q, 100)
    return lo, r, min(lo + (r > 0), n - 1)


def surface(target, prediction, label, defect=None):
    """dict: flags uint8, counts[5], d2T / d2P int64, hist int64[hist_bins], result[12] python ints.  defect: one of
    DEFECTS, a deliberately wrong reading of the definitions (tests/test_surface_ref_cpu.py)."""
    assert defect is None or defect in DEFECTS
    T, P = target == label, prediction == label
    eb = defect == "edge_background"
    bT = border(T, S6 if defect == "border6" else S26, eb)
    bP = border(P, S6 if defect == "border6" else S26, eb)
    cT, cP = border(T, S6, eb), border(P, S6, eb)
    flags = (T * IN_T + P * IN_P + bT * B26_T + bP * B26_P + cT * C6_T + cP * C6_P).astype(np.uint8)
    counts = [int(T.sum()), int(P.sum()), int((T & P).sum()), int(cT.sum()), int(cP.sum())]
    d2T, d2P = d2_of(bT), d2_of(bP)
    nb = hist_bins(T.shape)
    valid = 0 < counts[0] < T.size and 0 < counts[1] < T.size
    hist = np.zeros(nb, np.int64)
    res = counts + [0] * 7
    if valid:
        S = np.concatenate([d2T[cP], d2P[cT]])
        hist = np.bincount(S, minlength=nb).astype(np.int64)
        S.sort()
        n = len(S)
        if defect == "hd_on_contours":
            hd2 = int(S[-1])
        else:
            hd2 = max(int(d2T[P & ~T].max(initial=0)), int(d2P[T & ~P].max(initial=0)), 0)
        lo, r, hi = select(n)
        if defect == "nearest_rank":
            lo = hi = math.ceil(0.95 * n) - 1
            r = 0
        res = counts + [hd2, n, int(S[lo]), int(S[hi]), lo, r, 1]
    return dict(flags=flags, counts=counts, d2T=d2T, d2P=d2P, hist=hist, result=res)


def scores(result):
    """the reference's five numbers (metrics.py:156-238, without the two error rates) in fp64 from result[12]"""
    nT, nP, nI, _c6t, _c6p, hd2, _n, slo, shi, _lo, r, valid = (int(v) for v in result)
    nan = float("nan")
    out = {"Jaccard": nI / (nT + nP - nI) if nT + nP - nI else nan,
           "Dice": 2 * nI / (nT + nP) if nT + nP else nan,
           "VolumeSimilarity": 2 * (nT - nP) / (nT + nP) if nT + nP else nan,
           "HausdorffDistance": nan, "HausdorffDistance95": nan}
    if valid:
        a, b = math.sqrt(slo), math.sqrt(shi)
        out["HausdorffDistance"] = math.sqrt(hd2)
        out["HausdorffDistance95"] = a + (b - a) * r / 100
    return out


# ------------------------------------------------------------------------------------------------------ inputs
def _sigma(shape, s):
    return tuple(min(s, max(d / 4.0, 0.25)) for d in shape)


def _field(shape, seed, s=2.5):
    """smoothed uniform noise, rescaled to rank order in [0, 1) so that a threshold is a fill fraction"""
    rng = np.random.default_rng(seed)
    f = ndi.gaussian_filter(rng.random(shape), _sigma(shape, s), mode="nearest")
    return f.ravel().argsort().argsort().reshape(shape) / f.size


def blobs(shape, seed, fill=0.12, label=1, noise=0.35):
    """(target, prediction) uint8: a thresholded gaussian_filter of uniform noise and a perturbed copy of it"""
    a, b = _field(shape, seed), _field(shape, seed + 1000)
    t = a >= 1 - fill
    mix = (1 - noise) * a + noise * b
    p = mix >= np.quantile(mix, 1 - fill)
    rng = np.random.default_rng(seed + 7)
    other = (rng.random(shape) < 0.05) * (label % 255 + 1)        # voxels of another class: never part of T or P
    tgt = np.where(t, label, other).astype(np.uint8)
    prd = np.where(p, label, other[::-1, ::-1, ::-1]).astype(np.uint8)
    return tgt, prd


def label_maps(shape, seed, n_cls):
    """(target, prediction) uint8 with labels 0..n_cls: quantised smooth fields"""
    a, b = _field(shape, seed, 4.0), _field(shape, seed + 1000, 4.0)
    cut = np.array([0.55, 0.75, 0.9, 0.96, 0.99][:n_cls])
    mix = 0.7 * a + 0.3 * b
    mix = mix.ravel().argsort().argsort().reshape(shape) / mix.size
    return np.digitize(a, cut).astype(np.uint8), np.digitize(mix, cut).astype(np.uint8)


# (2, 600, 5): a line of 512..1023 voxels, the one LDS tile width of the distance transform that the others do not reach
SHAPES = [(1, 1, 1), (1, 33, 70), (19, 67, 131), (5, 3, 300), (2, 3, 1024), (3, 1024, 2), (1024, 2, 3), (40, 48, 56),
          (2, 600, 5)]
MASKS = ["blobs", "faces", "identical", "corners", "distant", "empty_t", "empty_p", "empty_both", "full"]


@functools.lru_cache(maxsize=None)
def case(shape, kind):
    """(target, prediction, label) for one of MASKS on one of SHAPES; the arrays are shared: do not write to them"""
    z = np.zeros(shape, np.uint8)
    seed = 17 + sum(shape)
    if kind == "blobs":
        t, p = blobs(shape, seed, 0.12, label=3)
        return t, p, 3
    if kind == "faces":                      # large objects that run into the volume's faces
        t, p = blobs(shape, seed + 1, 0.45, label=255)
        return t, p, 255
    if kind == "identical":
        t, _ = blobs(shape, seed + 2, 0.2)
        return t, t.copy(), 1
    if kind == "corners":
        t, p = z.copy(), z.copy()
        t[0, 0, 0] = 1
        p[-1, -1, -1] = 1
        return t, p, 1
    if kind == "distant":                    # two objects at opposite ends of the longest axis
        t, p = z.copy(), z.copy()
        ax = int(np.argmax(shape))
        k = max(1, shape[ax] // 5)
        sl = [slice(None)] * 3
        sl[ax] = slice(0, k)
        t[tuple(sl)] = 1
        sl[ax] = slice(shape[ax] - k, None)
        p[tuple(sl)] = 1
        return t, p, 1
    t, p = blobs(shape, seed + 3, 0.2)
    if kind == "empty_t":
        return z, p, 1
    if kind == "empty_p":
        return t, z, 1
    if kind == "empty_both":
        return z, z.copy(), 1
    if kind == "full":
        return z + 1, p, 1
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def case_ref(shape, kind):
    t, p, k = case(shape, kind)
    return surface(t, p, k)


def seed_sets(shape):
    """{name: bool seed array} for hdf_op_edt_sq on its own: a single seed, none, seeds on one face only"""
    one = np.zeros(shape, bool)
    one[tuple(s // 3 for s in shape)] = True
    face = np.zeros(shape, bool)
    face[..., 0] = np.random.default_rng(5).random(shape[:2]) < 0.3
    face[0, 0, 0] = True
    return {"single": one, "none": np.zeros(shape, bool), "face": face}
