"""The physical-unit surface-distance definitions of include/hdf.h restated in fp64 numpy (no GPU part), and the planted
defects the GPU tests' inputs must be able to see.  Cases, masks and flags are tests/surface_ref.py's and tests/asd_ref.py's;
only the metric is new.

spacing = (sz, sy, sx) in the axis order of the [D][H][W] array, weights w = fl(s s).  For a seed set M
    D2_M(v) = min over u in M of fl( fl(wz a^2) + fl( fl(wy b^2) + fl(wx c^2) ) ),   (a, b, c) = |v - u|,
+inf where M is empty.  `d2_mm` forms it the way the kernels do -- c^2 along W as an integer, then a pass along H, then one
along D -- and tests/test_surface_mm_ref_cpu.py holds it to a brute force over all seeds in every bit.  numpy rounds every
product and every sum on its own (it never fuses them), which is what the definition asks for."""
import functools
import math
import struct

import numpy as np
from scipy import ndimage as ndi

import asd_ref as ar
import surface_ref as sr

SPACINGS = [(1.0, 1.0, 1.0), (3.0, 0.5, 0.5), (0.5, 0.5, 3.0), (0.7, 1.3, 2.9), (2.5, 1.0, 1.0)]
DEFECTS = ("wrong_axes", "not_squared", "voxel_nearest", "hi_distinct", "rank_off", "sum_fp32")
INF = float("inf")


def bits(x):
    """the IEEE fp64 bit pattern of x as a non-negative python int"""
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def unbits(b):
    return struct.unpack("<d", struct.pack("<Q", int(b) & 0xFFFFFFFFFFFFFFFF))[0]


def weights(spacing):
    return tuple(np.float64(s) * np.float64(s) for s in spacing)


def row_c2(seed):
    """int64 squared index distance to the nearest seed along the last axis; sr.NO_SEED where the row holds none"""
    w = seed.shape[-1]
    far = 1 << 20
    idx = np.arange(w, dtype=np.int64)
    left = np.maximum.accumulate(np.where(seed, idx, -far), axis=-1)
    right = np.minimum.accumulate(np.where(seed, idx, far)[..., ::-1], axis=-1)[..., ::-1]
    d = np.minimum(idx - left, right - idx)
    return np.where(d >= far // 2, sr.NO_SEED, d * d)


def col_pass(f, w, axis):
    """g(i) = min_j fl(f(j) + fl(w (i - j)^2)) along `axis` of the fp64 array f (+inf: nothing yet)"""
    f = np.moveaxis(f, axis, 0)
    n = f.shape[0]
    out = np.full(f.shape, INF)
    i = np.arange(n, dtype=np.int64)
    for j in range(n):
        if not np.isfinite(f[j]).any():
            continue
        q = w * ((i - j) ** 2).astype(np.float64)                 # one rounding a product
        out = np.minimum(out, f[j][None] + q.reshape((n,) + (1,) * (f.ndim - 1)))   # one rounding a sum
    return np.moveaxis(out, 0, axis)


def d2_mm(seed, spacing):
    """fp64 D2_M of every voxel for the boolean seed array M; +inf everywhere when M is empty"""
    wz, wy, wx = weights(spacing)
    c2 = row_c2(seed)
    f = np.where(c2 >= sr.NO_SEED, INF, wx * c2.astype(np.float64))
    return col_pass(col_pass(f, wy, 1), wz, 0)


def d2_brute(seed, spacing):
    """the definition itself: a minimum over all seeds, every product and sum rounded once, in the order written there"""
    wz, wy, wx = weights(spacing)
    out = np.full(seed.shape, INF)
    z, y, x = (g.astype(np.int64) for g in np.indices(seed.shape))
    for u in np.argwhere(seed):
        a2, b2, c2 = ((z - u[0]) ** 2).astype(np.float64), ((y - u[1]) ** 2).astype(np.float64), \
            ((x - u[2]) ** 2).astype(np.float64)
        out = np.minimum(out, wz * a2 + (wy * b2 + wx * c2))
    return out


def _d2(seed, spacing, defect):
    if defect == "wrong_axes":
        return d2_mm(seed, (spacing[1], spacing[2], spacing[0]))
    if defect == "not_squared":
        return d2_mm(seed, tuple(math.sqrt(s) for s in spacing))
    if defect == "voxel_nearest" and seed.any():                  # the nearest seed in voxels, its distance in millimetres
        idx = ndi.distance_transform_edt(~seed, return_distances=False, return_indices=True).astype(np.int64)
        a2, b2, c2 = (((idx[k] - g) ** 2).astype(np.float64) for k, g in enumerate(np.indices(seed.shape)))
        wz, wy, wx = weights(spacing)
        return wz * a2 + (wy * b2 + wx * c2)
    return d2_mm(seed, spacing)


def surface(target, prediction, label, spacing, defect=None, base=None):
    """dict: flags, counts, d2T / d2P fp64, S (sorted fp64), result[12] python ints laid out like hdf_surface_distances
    with words 5, 7, 8 as bit patterns.  base: sr.surface(target, prediction, label) where the caller has it already."""
    assert defect is None or defect in DEFECTS
    base = base or sr.surface(target, prediction, label)
    flags, counts = base["flags"], base["counts"]
    T, P = (flags & sr.IN_T) != 0, (flags & sr.IN_P) != 0
    cT, cP = (flags & sr.C6_T) != 0, (flags & sr.C6_P) != 0
    d2T, d2P = _d2((flags & sr.B26_T) != 0, spacing, defect), _d2((flags & sr.B26_P) != 0, spacing, defect)
    valid = 0 < counts[0] < T.size and 0 < counts[1] < T.size
    res, S = counts + [0] * 7, np.zeros(0)
    if valid:
        S = np.sort(np.concatenate([d2T[cP], d2P[cT]]))
        n = len(S)
        hd2 = max(float(d2T[P & ~T].max(initial=0.0)), float(d2P[T & ~P].max(initial=0.0)), 0.0)
        lo, r, hi = sr.select(n)
        if defect == "rank_off":
            lo, hi = min(lo + 1, n - 1), min(hi + 1, n - 1)
        shi = S[hi]
        if defect == "hi_distinct" and hi > lo:
            above = S[S > S[lo]]
            shi = above[0] if len(above) else S[lo]
        res = counts + [bits(hd2), n, bits(S[lo]), bits(shi), sr.select(n)[0], r, 1]
    return dict(flags=flags, counts=counts, d2T=d2T, d2P=d2P, S=S, result=res)


def scores(result):
    """the five numbers in fp64 from result[12], the way hdf_rt.surface.scores_from_result_mm forms them"""
    row = list(result)
    for k in (5, 7, 8):
        row[k] = unbits(row[k])
    nT, nP, nI, _c6t, _c6p, hd2, _n, slo, shi, _lo, r, valid = row
    out = sr.scores([nT, nP, nI, 0, 0, 0, 0, 0, 0, 0, 0, 0])
    if valid:
        a, b = math.sqrt(slo), math.sqrt(shi)
        out["HausdorffDistance"] = math.sqrt(hd2)
        out["HausdorffDistance95"] = a + (b - a) * r / 100
    return out


def asd(target, prediction, label, spacing, defect=None, base=None):
    """dict: flags, counts [|E6(T)|, |E6(P)|], d2ET / d2EP fp64, sumA / sumB (math.fsum), result[4], scores"""
    assert defect is None or defect in DEFECTS
    base = base or ar.asd(target, prediction, label)
    flags, counts = base["flags"], base["counts"]
    eT, eP = (flags & ar.E6_T) != 0, (flags & ar.E6_P) != 0
    d2ET, d2EP = _d2(eT, spacing, defect), _d2(eP, spacing, defect)
    sA = sB = 0.0
    if counts[0] and counts[1]:                   # otherwise one map is all +inf: there are no distances
        if defect == "sum_fp32":
            sA = float(np.cumsum(np.sqrt(d2ET[eP]).astype(np.float32), dtype=np.float32)[-1])
            sB = float(np.cumsum(np.sqrt(d2EP[eT]).astype(np.float32), dtype=np.float32)[-1])
        else:
            sA, sB = math.fsum(np.sqrt(d2ET[eP]).tolist()), math.fsum(np.sqrt(d2EP[eT]).tolist())
    return dict(flags=flags, counts=counts, d2ET=d2ET, d2EP=d2EP, sumA=sA, sumB=sB,
                result=counts + [bits(sA), bits(sB)], scores=ar.floats(counts[0], counts[1], sA, sB))


def select_ref(keys, lo, defect=None):
    """(sorted[lo], sorted[min(lo + 1, n - 1)]) of a uint64 array: what hdf_op_select_u64 returns"""
    s = np.sort(np.asarray(keys, np.uint64))
    n = len(s)
    if defect == "rank_off":
        lo = min(lo + 1, n - 1)
    second = s[min(lo + 1, n - 1)]
    if defect == "hi_distinct":
        above = s[s > s[lo]]
        second = above[0] if len(above) else s[lo]
    return int(s[lo]), int(second)


@functools.lru_cache(maxsize=None)
def select_cases():
    """[(name, uint64 keys, ranks)]: the crafted key sets of hdf_op_select_u64; shared: do not write to the arrays"""
    rng = np.random.default_rng(11)
    base = bits(1234.5678)
    out = [("n=1", np.array([base], np.uint64), [0]),
           ("all equal", np.full(777, base, np.uint64), [0, 388, 776]),
           ("two values", np.array([7] * 5 + [9] * 3, np.uint64)[rng.permutation(8)], list(range(8))),
           ("lowest bit", (np.uint64(base) ^ (rng.integers(0, 2, 3000).astype(np.uint64))), [0, 1499, 2849, 2999])]
    for digit in range(4):                   # keys that differ in exactly one 16-bit digit of the 64
        d = rng.integers(0, 1 << 16, 5000).astype(np.uint64) << np.uint64(16 * digit)
        keep = np.uint64(base) & ~(np.uint64(0xFFFF) << np.uint64(16 * digit))
        out.append((f"digit {digit}", keep | d, [0, 1, 2500, 4749, 4998, 4999]))
    # the bit patterns of random non-negative doubles over many binades, a few of them repeated, zero and +inf among them
    r = np.abs(rng.standard_normal(70000) * np.exp(rng.uniform(-30, 30, 70000)))
    r[:500] = r[500:1000]
    r[1000], r[1001] = 0.0, np.inf
    n = len(r)
    out.append(("random", r.view(np.uint64).copy(), [0, n - 1, sr.select(n)[0], sr.select(n)[0] + 1, n // 2]))
    return out


@functools.lru_cache(maxsize=None)
def case_ref(shape, kind, spacing):
    """surface() of surface_ref.case(shape, kind) with `spacing`; shared: do not write to its arrays"""
    t, p, k = sr.case(shape, kind)
    return surface(t, p, k, spacing, base=sr.case_ref(shape, kind))


@functools.lru_cache(maxsize=None)
def asd_case_ref(shape, kind, spacing):
    t, p, k = sr.case(shape, kind)
    return asd(t, p, k, spacing, base=ar.case_ref(shape, kind))
