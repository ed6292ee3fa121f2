"""The order statistics of include/hdf.h (hdf_cc_quantiles) restated with numpy (no GPU part), and the one comparison both
the GPU test and the planted-defect test use.

quantiles(ids, image, q, capacity) gives, per id in 1..capacity (row id - 1; a value below 0 counts as 0, ids above capacity
are left out): count = n by np.bincount; per channel the values of the id sorted (np.lexsort by id and value: np.sort per
id, all ids at once), a -0 read as +0; per level q, in fp64, h = q * (n - 1) (one multiplication), lo = floor(h), frac = h -
lo (exact), hi = lo + (frac > 0), and the three numbers s_lo, s_hi, s_lo + frac * (s_hi - s_lo) -- numpy rounds after the
subtraction, after the multiplication and after the addition, and fuses nothing.  Rows no voxel holds are zeros.  result is
measure_ref's.

Nothing here has a tolerance: the device selects exact order statistics with integer counts and forms the third number
with the same three roundings, so mismatches() asks for every output byte."""
import numpy as np

LEVELS16 = (0.5, 0.0, 1.0, 1.0 / 3.0, 0.95, 0.5, 0.25, 0.1, 0.9, 0.0, 0.75, 0.999, 0.001, 2.0 / 3.0, 0.05, 1.0)


def ranks(n, q):
    """(lo int64, hi int64, frac fp64) of the definition for counts n (an array, each at least 1) and one level q"""
    h = np.float64(q) * (np.asarray(n, np.int64) - 1).astype(np.float64)
    lo = np.floor(h)
    frac = h - lo
    return lo.astype(np.int64), lo.astype(np.int64) + (frac > 0), frac


def quantiles(ids, image, q, capacity):
    """dict(count int64 [cap], values fp64 [C, cap, Q, 3], result [4]).  ids [D, H, W] integers, image [C, D, H, W] float32,
    q a sequence of levels in [0, 1]."""
    ids = np.asarray(ids)
    image = np.asarray(image, np.float32)
    assert ids.ndim == 3 and image.ndim == 4 and image.shape[1:] == ids.shape
    q = [float(v) for v in q]
    assert q and all(0.0 <= v <= 1.0 for v in q)
    C, cap, Q = image.shape[0], int(capacity), len(q)
    flat = np.where(ids.ravel() < 0, 0, ids.ravel()).astype(np.int64)
    result = [int(flat.max()), int(np.count_nonzero(flat > 0)), int(np.count_nonzero((flat > 0) & (flat <= cap))), 0]
    vox = np.flatnonzero((flat > 0) & (flat <= cap))
    row = flat[vox] - 1
    count = np.bincount(row, minlength=cap).astype(np.int64)
    values = np.zeros((C, cap, Q, 3))
    present = np.flatnonzero(count)
    start = (np.cumsum(count) - count)[present]
    n = count[present]
    for c in range(C):
        val = image[c].ravel()[vox] + np.float32(0.0)             # -0 + 0 = +0
        s = val[np.lexsort((val, row))].astype(np.float64)       # by id, within an id ascending: np.sort of every id
        for k, level in enumerate(q):
            lo, hi, frac = ranks(n, level)
            s_lo, s_hi = s[start + lo], s[start + hi]
            d = s_hi - s_lo
            p = frac * d
            values[c, present, k, 0], values[c, present, k, 1], values[c, present, k, 2] = s_lo, s_hi, s_lo + p
    return dict(count=count, values=values, result=result)


def mismatches(got, want):
    """names of what differs between a dict of the device's outputs (count, values, result) and quantiles()'s: every output
    byte must agree (a -0 for a +0 is a mismatch).  The comparison of the GPU test, and the one the planted defects must
    not get past."""
    bad = []
    if [int(v) for v in got["result"]] != [int(v) for v in want["result"]]:
        bad.append("result")
    n = np.ascontiguousarray(got["count"], np.int64)
    if n.shape != want["count"].shape:
        return bad + ["count.shape"]
    if n.tobytes() != want["count"].tobytes():
        bad.append("count")
    v = np.ascontiguousarray(got["values"], np.float64)
    if v.shape != want["values"].shape:
        return bad + ["values.shape"]
    for k, name in enumerate(("lower", "upper", "value")):
        if np.ascontiguousarray(v[..., k]).tobytes() != np.ascontiguousarray(want["values"][..., k]).tobytes():
            bad.append(name)
    absent = want["count"] == 0
    if v[:, absent].view(np.int64).any() or n[absent].any():
        bad.append("absent rows")
    return bad
