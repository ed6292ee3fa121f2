"""The region measurements of include/hdf.h (hdf_cc_measure) restated with numpy and math.fsum (no GPU part), the inputs of
the GPU tests and the one comparison both the GPU test and the planted-defect test use.

measure(ids, image, capacity) gives, per id in 1..capacity (row id - 1; a value below 0 counts as 0, ids above capacity are
left out): geom = n, sum z, sum y, sum x by np.bincount; per channel, over the voxels of the id in ascending linear index
(a stable sort), S1 = fsum(x), mean = S1 / n, M2 = fsum((x - mean)^2), min, max, the first index of each (np.argmin /
np.argmax), Wz / Wy / Wx = fsum(z x) ...; a -0 is read as +0; rows no voxel holds are zeros.  fsum is exactly rounded, and
the products z x are exact in fp64 (10 + 24 bits).

The bounds of mismatches() are derived, not measured.  u = 2^-53, n = the voxels of the component.
  sums   The device adds n exact terms t in some fixed order.  Every addition rounds once, |fl(a + b) - (a + b)| <=
         u |a + b|, and a term passes through at most n - 1 additions, so |got - sum t| <= ((1 + u)^(n-1) - 1) sum|t|, which
         is (n - 1) u sum|t| up to a factor 1 + n u.  The restatement's fsum is within u |sum t| <= u sum|t| of the same
         value.  Together: n u sum|t|.
  mean   got = fl(S1' / n) with S1' the device's sum: |S1' - S1| / n from the sum plus one rounding u |mean| (the
         restatement's own rounding of the quotient is inside the same u |mean| to second order): n u sum|x| / n + u |mean|.
  M2     With m' the device's mean and m the exact one, sum (x - m')^2 = sum (x - m)^2 + n (m - m')^2 because the cross term
         sum (x - m) vanishes; |m - m'| <= (n + 1) u sum|x| / n by the line above.  Each term then carries the rounding of
         x - m' and of the square (or of the fused multiply-add), and the sum n - 1 more: (n + 2) u M2 to first order.  The
         restatement rounds its own mean and terms in the same way, hence the factor 2:
         2 [(n + 2) u M2 + n ((n + 1) u sum|x| / n)^2].
Integers, min, max, pos and result are compared exactly (min and max by their bits: a -0 is a mismatch)."""
import functools
import math

import numpy as np

import cc_ref

U = 2.0 ** -53
STAT_COLS = ("sum", "mean", "m2", "min", "max", "wz", "wy", "wx")


def measure(ids, image, capacity):
    """dict(geom int64 [cap, 4], stats fp64 [C, cap, 8], pos int64 [C, cap, 2], result [4], abs fp64 [C, cap, 4] = the sums of
    |x|, |z x|, |y x|, |x x| that the bounds need).  ids [D, H, W] integers, image [C, D, H, W] float32."""
    ids = np.asarray(ids)
    image = np.asarray(image, np.float32)
    assert ids.ndim == 3 and image.ndim == 4 and image.shape[1:] == ids.shape
    C, cap = image.shape[0], int(capacity)
    flat = np.where(ids.ravel() < 0, 0, ids.ravel()).astype(np.int64)
    result = [int(flat.max()), int(np.count_nonzero(flat > 0)), int(np.count_nonzero((flat > 0) & (flat <= cap))), 0]
    vox = np.flatnonzero((flat > 0) & (flat <= cap))
    row = flat[vox] - 1
    z, y, x = (a.astype(np.int64) for a in np.unravel_index(vox, ids.shape))
    geom = np.zeros((cap, 4), np.int64)
    geom[:, 0] = np.bincount(row, minlength=cap)
    for k, coord in enumerate((z, y, x), 1):
        np.add.at(geom[:, k], row, coord)
    stats, pos, ab = np.zeros((C, cap, 8)), np.zeros((C, cap, 2), np.int64), np.zeros((C, cap, 4))
    order = np.argsort(row, kind="stable")                       # within an id the voxels stay in ascending linear index
    vox, row, coords = vox[order], row[order], [a[order].astype(np.float64) for a in (z, y, x)]
    present = np.flatnonzero(geom[:, 0])
    start = np.searchsorted(row, present)
    n_of = geom[present, 0]
    for c in range(C):
        val = image[c].ravel()[vox].astype(np.float64) + 0.0     # -0 + 0 = +0
        one = n_of == 1                                          # components of one voxel, all at once
        r1, s1 = present[one], start[one]
        v1 = val[s1]
        stats[c, r1, 0], stats[c, r1, 1], stats[c, r1, 3], stats[c, r1, 4] = v1, v1, v1, v1
        pos[c, r1, 0], pos[c, r1, 1] = vox[s1], vox[s1]
        ab[c, r1, 0] = np.abs(v1)
        for k in range(3):
            stats[c, r1, 5 + k] = coords[k][s1] * v1 + 0.0       # (0 * a negative value: a sum that is zero is +0, as fsum's)
            ab[c, r1, 1 + k] = np.abs(coords[k][s1] * v1)
        for r, s, n in zip(present[~one].tolist(), start[~one].tolist(), n_of[~one].tolist()):
            v = val[s: s + n]
            s1_ = math.fsum(v.tolist()) + 0.0
            mean = s1_ / n
            d = v - mean
            lo, hi = int(np.argmin(v)), int(np.argmax(v))
            stats[c, r, :5] = s1_, mean, math.fsum((d * d).tolist()), v[lo], v[hi]
            pos[c, r] = vox[s + lo], vox[s + hi]
            ab[c, r, 0] = np.abs(v).sum()
            for k in range(3):
                t = coords[k][s: s + n] * v
                stats[c, r, 5 + k] = math.fsum(t.tolist()) + 0.0
                ab[c, r, 1 + k] = np.abs(t).sum()
    return dict(geom=geom, stats=stats, pos=pos, result=result, abs=ab)


def bounds(want):
    """fp64 [C, cap, 8]: the allowance of every column of stats (0 for min and max), from the restatement alone"""
    n = want["geom"][:, 0].astype(np.float64)[None, :]
    st, ab = want["stats"], want["abs"]
    b = np.zeros_like(st)
    b[..., 0] = n * U * ab[..., 0]
    safe = np.maximum(n, 1.0)
    b[..., 1] = b[..., 0] / safe + U * np.abs(st[..., 1])
    b[..., 2] = 2.0 * ((n + 2.0) * U * st[..., 2] + n * ((n + 1.0) * U * ab[..., 0] / safe) ** 2)
    for k in range(3):
        b[..., 5 + k] = n * U * ab[..., 1 + k]
    return b


def mismatches(got, want):
    """names of what differs between a dict of the device's outputs (geom, stats, pos, result) and measure()'s: integers, min,
    max, pos and result exactly, the fp64 sums to bounds(); the comparison of the GPU test, and the one the planted defects
    must not get past"""
    bad = []
    if [int(v) for v in got["result"]] != [int(v) for v in want["result"]]:
        bad.append("result")
    g = np.asarray(got["geom"], np.int64)
    if g.shape != want["geom"].shape:
        return bad + ["geom.shape"]
    for k, name in enumerate(("n", "sum_z", "sum_y", "sum_x")):
        if not np.array_equal(g[:, k], want["geom"][:, k]):
            bad.append(name)
    if not np.array_equal(np.asarray(got["pos"], np.int64)[..., 0], want["pos"][..., 0]):
        bad.append("argmin")
    if not np.array_equal(np.asarray(got["pos"], np.int64)[..., 1], want["pos"][..., 1]):
        bad.append("argmax")
    s = np.ascontiguousarray(got["stats"], np.float64)
    if s.shape != want["stats"].shape:
        return bad + ["stats.shape"]
    for k in (3, 4):
        if not np.array_equal(s[..., k].copy().view(np.int64), want["stats"][..., k].copy().view(np.int64)):
            bad.append(STAT_COLS[k])
    b = bounds(want)
    for k in (0, 1, 2, 5, 6, 7):
        err = np.abs(s[..., k] - want["stats"][..., k])
        if not bool((err <= b[..., k]).all()):                   # (a NaN compares false: a NaN output fails)
            bad.append(STAT_COLS[k])
    absent = want["geom"][:, 0] == 0
    if s[:, absent].view(np.int64).any() or np.asarray(got["pos"])[:, absent].any() or g[absent].any():
        bad.append("absent rows")
    return bad


def worst(got, want):
    """the largest error / bound over the fp64 sums (0 / 0 counts as 0): printed by the tests before they assert"""
    b = bounds(want)
    err = np.abs(np.asarray(got["stats"], np.float64) - want["stats"])
    cols = [0, 1, 2, 5, 6, 7]
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err[..., cols] == 0, 0.0, err[..., cols] / b[..., cols])
    return float(ratio.max()) if ratio.size else 0.0


def _div(a, b):
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.float64(a) / np.float64(b))


def dicts(want, shape, spacing=None):
    """what hdf_rt.region_stats returns, from measure()'s arrays: one dict per id that is present"""
    _, H, W = shape
    out = []
    for r in np.flatnonzero(want["geom"][:, 0]).tolist():
        n, sz, sy, sx = (int(v) for v in want["geom"][r])
        d = {"id": r + 1, "size": n, "centroid": (sz / n, sy / n, sx / n), "channels": []}
        if spacing is not None:
            d["volume_mm3"] = n * spacing[0] * spacing[1] * spacing[2]
            d["centroid_mm"] = tuple(c * s for c, s in zip(d["centroid"], spacing))
        for c in range(want["stats"].shape[0]):
            s1, mean, m2, lo, hi, wz, wy, wx = (float(v) for v in want["stats"][c, r])
            com = (_div(wz, s1), _div(wy, s1), _div(wx, s1))
            ch = {"sum": s1, "mean": mean, "variance": m2 / n, "std": math.sqrt(m2 / n), "min": lo, "max": hi,
                  "argmin": tuple(int(v) for v in np.unravel_index(int(want["pos"][c, r, 0]), shape)),
                  "argmax": tuple(int(v) for v in np.unravel_index(int(want["pos"][c, r, 1]), shape)), "center_of_mass": com}
            if spacing is not None:
                ch["center_of_mass_mm"] = tuple(a * s for a, s in zip(com, spacing))
            d["channels"].append(ch)
        out.append(d)
    return out


# ------------------------------------------------------------------------------------------------------ inputs
# (19, 67, 131): odd on every axis, 166 763 voxels; as ONE component each of its eight slabs is 20 846 voxels, 82 trips of a
# workgroup, the last slab 20 841.  (5, 3, 300): a row longer than the 256 lanes of a workgroup.  1024 on each axis in turn.
SHAPES = [(1, 1, 1), (1, 37, 70), (19, 67, 131), (5, 3, 300), (1024, 3, 5), (3, 1024, 5), (3, 5, 1024)]
BIG = (19, 67, 131)
IMAGES = ["uniform", "signed", "constant", "ints", "levels", "zeros_denormals"]
MASKS = ["rand20", "rand50", "rand80", "empty", "full", "checker", "serpentine"]


@functools.lru_cache(maxsize=None)
def image(kind, shape, C):
    """float32 [C, D, H, W]; shared: do not write to it"""
    rng = np.random.default_rng(7 + sum(shape) * 31 + C + len(kind))
    full = (C,) + tuple(shape)
    if kind == "uniform":                    # [0, 1)
        a = rng.random(full, dtype=np.float32)
    elif kind == "signed":                   # both signs, exponents spread over 2^-20 .. 2^20
        a = (rng.uniform(1.0, 2.0, full) * np.exp2(rng.integers(-20, 21, full)) * rng.choice([-1.0, 1.0], full)).astype(np.float32)
    elif kind == "constant":
        a = np.full(full, np.float32(0.7), np.float32)
    elif kind == "ints":                     # small integers, negative ones included: every sum is exact
        a = rng.integers(-50, 200, full).astype(np.float32)
    elif kind == "levels":                   # four levels: every extremum is tied many times
        a = np.asarray([-1.5, 0.25, 0.25 + 2.0 ** -20, 3.0], np.float32)[rng.integers(0, 4, full)]
    elif kind == "zeros_denormals":          # +0, -0, the smallest denormals of both signs, the largest denormal, FLT_MIN
        bits = np.asarray([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x00800000, 0x80000002], np.uint32)
        a = bits[rng.integers(0, len(bits), full)].view(np.float32)
    else:
        raise KeyError(kind)
    a = np.ascontiguousarray(a, np.float32)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def labelled(shape, kind, connectivity):
    """(ids int32, n): one of cc_ref's masks labelled on the host"""
    ids, n = cc_ref.label(cc_ref.case(shape, kind), connectivity, 0)
    ids.setflags(write=False)
    return ids, n


@functools.lru_cache(maxsize=None)
def special_ids(shape, kind):
    """(ids int32, the largest id): numberings that are not a labelling's"""
    rng = np.random.default_rng(101 + sum(shape))
    V = int(np.prod(shape))
    if kind == "gaps":                       # ids 3, 4, 9 and 40 in slabs of the linear order, -7 and 0 between them
        ids = np.asarray([0, 3, -7, 9, 4, 0, 40, 9], np.int32)[(np.arange(V) * 8 // max(V, 1)) % 8]
        ids = np.where(rng.random(V) < 0.3, 0, ids).astype(np.int32)
        if V >= 8:
            ids[V // 2] = -2_000_000_000
    elif kind == "classes":                  # a three-class map widened to int32
        ids = rng.integers(0, 4, V).astype(np.int32)
    elif kind == "tiny":                     # components of 1 and of 3 voxels (fewer than slabs), far apart
        ids = np.zeros(shape, np.int32)
        if min(shape) >= 3:                  # three voxels in three planes, rows and columns: a box far larger than the component
            ids[0, shape[1] - 1, 1] = ids[1, 0, shape[2] - 1] = ids[2, 1, 0] = 5
        ids = ids.ravel()
        ids[0] = 1
        if V >= 8:
            ids[V - 1] = 2
            ids[[V // 3, V // 3 + 1, V // 3 + 2]] = 3
    else:
        raise KeyError(kind)
    ids = ids.reshape(shape)
    ids.setflags(write=False)
    return ids, int(max(ids.max(), 0))


@functools.lru_cache(maxsize=None)
def reference(shape, ids_key, image_kind, C, capacity):
    """measure() of one case; ids_key = ("label", mask kind, connectivity) or ("special", kind).  Shared: do not write."""
    ids = labelled(shape, ids_key[1], ids_key[2])[0] if ids_key[0] == "label" else special_ids(shape, ids_key[1])[0]
    return measure(ids, image(image_kind, shape, C), capacity)
