"""The connected-component definitions of include/hdf.h restated with scipy (no GPU part), the inputs of the GPU tests
and the one comparison both the GPU test and the planted-defect test use.

Two voxels are adjacent when they are neighbours under the connectivity (6 / 18 / 26 = generate_binary_structure(3, 1 / 2 /
3)) and hold the same non-zero value.  label = 0 takes every non-zero value, label = k the voxels equal to k.  Ids are
1..n in ascending order of each component's smallest linear voxel index: per value that is ndimage.label's own numbering,
across values the per-value labels are renumbered by first voxel."""
import functools

import numpy as np
from scipy import ndimage as ndi

STRUCTURE = {6: ndi.generate_binary_structure(3, 1), 18: ndi.generate_binary_structure(3, 2),
             26: ndi.generate_binary_structure(3, 3)}
CONNECTIVITIES = (6, 18, 26)
COLS = ("size", "value", "first", "zmin", "zmax", "ymin", "ymax", "xmin", "xmax")


def label(vol, connectivity=26, label=0):
    """(ids int32 like vol, n)"""
    values = [label] if label else [int(u) for u in np.unique(vol) if u]
    firsts, owner, labs = [], [], {}
    for u in values:
        lab, k = ndi.label(vol == u, STRUCTURE[connectivity])
        labs[u] = lab
        if k:
            ids_u, first = np.unique(lab.ravel(), return_index=True)      # sorted by local id; [0] is the background
            keep = ids_u > 0
            assert np.array_equal(ids_u[keep], np.arange(1, k + 1))
            assert (np.diff(first[keep]) > 0).all()                        # scipy numbers by first voxel
            firsts += first[keep].tolist()
            owner += [(u, int(i)) for i in ids_u[keep]]
    order = np.argsort(np.asarray(firsts, np.int64), kind="stable")
    ids = np.zeros(vol.shape, np.int32)
    maps = {u: np.zeros(int(labs[u].max()) + 1, np.int32) for u in values}
    for new, j in enumerate(order, 1):
        u, local = owner[j]
        maps[u][local] = new
    for u in values:
        ids = np.where(vol == u, maps[u][labs[u]], ids).astype(np.int32)
    return ids, len(order)


def table(vol, ids, n, score=None):
    """(int64 [n, 9] in COLS order, float32 [n] or None)"""
    t = np.zeros((n, 9), np.int64)
    if n == 0:
        return t, (None if score is None else np.zeros(0, np.float32))
    index = np.arange(1, n + 1)
    t[:, 0] = np.rint(ndi.sum(np.ones(vol.shape), ids, index)).astype(np.int64)
    _, first = np.unique(ids.ravel(), return_index=True)
    first = first[-n:]                                                    # without the background's entry, if any
    t[:, 2] = first
    t[:, 1] = vol.ravel()[first]
    for i, sl in enumerate(ndi.find_objects(ids, max_label=n)):
        t[i, 3:] = [sl[0].start, sl[0].stop - 1, sl[1].start, sl[1].stop - 1, sl[2].start, sl[2].stop - 1]
    smax = None if score is None else np.asarray(ndi.maximum(score, ids, index), np.float32)
    return t, smax


def filter_map(vol, ids, sizes, values, min_size, keep_largest):
    """(out uint8, [components kept, voxels kept]) from the size list with np.argmax"""
    sizes, values = np.asarray(sizes, np.int64), np.asarray(values, np.int64)
    keep = sizes >= min_size
    if keep_largest:
        largest = np.zeros(len(sizes), bool)
        for u in np.unique(values):
            idx = np.flatnonzero(values == u)
            largest[idx[np.argmax(sizes[idx])]] = True                    # the first of equal sizes
        keep &= largest
    lut = np.concatenate([[False], keep])
    out = np.where(lut[ids], vol, 0).astype(np.uint8)
    return out, [int(keep.sum()), int(np.count_nonzero(lut[ids]))]


def min_sizes(sizes):
    """the four thresholds of the filter check: 0, 1, the size of the second largest component, that size + 1"""
    s = sorted((int(v) for v in sizes), reverse=True)
    second = s[1] if len(s) > 1 else 0
    return [0, 1, second, second + 1]


def full(vol, connectivity, lab, score=None):
    """everything the GPU test compares for one (volume, connectivity, label): ids, result, table, score_max and the
    eight filtered maps with their results"""
    ids, n = label(vol, connectivity, lab)
    t, smax = table(vol, ids, n, score)
    out = dict(ids=ids, result=[n, int(np.count_nonzero(ids))], table=t, score_max=smax, min_sizes=min_sizes(t[:, 0]),
               filters={})
    for ms in out["min_sizes"]:
        for kl in (0, 1):
            out["filters"][(ms, kl)] = filter_map(vol, ids, t[:, 0], t[:, 1], ms, kl)
    return out


def mismatches(got, want):
    """names of what differs between two dicts shaped like full()'s -- every element compared exactly (score_max bit for
    bit); the comparison of the GPU test, and the one the planted defects must not get past"""
    bad = []
    if not np.array_equal(np.asarray(got["ids"], np.int64), np.asarray(want["ids"], np.int64)):
        bad.append("ids")
    if [int(v) for v in got["result"]] != [int(v) for v in want["result"]]:
        bad.append("result")
    if "table" in got and not np.array_equal(np.asarray(got["table"], np.int64), want["table"]):
        bad.append("table")
    if got.get("score_max") is not None and want["score_max"] is not None:
        a, b = np.asarray(got["score_max"], np.float32), np.asarray(want["score_max"], np.float32)
        if a.shape != b.shape or not np.array_equal(a.view(np.int32), b.view(np.int32)):
            bad.append("score_max")
    for key, (out, res) in want["filters"].items():
        if key not in got.get("filters", {}):
            continue
        gout, gres = got["filters"][key]
        if not np.array_equal(np.asarray(gout, np.uint8), out):
            bad.append("filter%s.out" % (key,))
        if [int(v) for v in gres] != res:
            bad.append("filter%s.result" % (key,))
    return bad


# ------------------------------------------------------------------------------------------------------ inputs
SHAPES = [(1, 1, 1), (1, 37, 70), (19, 67, 131), (5, 3, 300), (1024, 2, 3), (2, 1024, 3), (3, 2, 1024), (40, 48, 56)]
MASKS = ["rand20", "rand50", "rand80", "empty", "full", "checker", "serpentine", "comb", "edge_corner", "wrap", "planes2",
         "tie"]
THREE_VALUES = (40, 48, 56)       # the shape whose random fills carry three values, in slabs along z


def _inside(shape, p):
    return all(0 <= c < s for c, s in zip(p, shape))


def serpentine(shape):
    """one path through the volume: whole rows on the even (z, y), run back and forth along x, joined to the next row and
    the next plane by a single voxel at the turn"""
    D, H, W = shape
    m = np.zeros(shape, np.uint8)
    forward, prev = True, None
    for zi, z in enumerate(range(0, D, 2)):
        ys = list(range(0, H, 2))
        for y in (ys if zi % 2 == 0 else ys[::-1]):
            if prev is not None:                                   # the connector between the previous row's end and this row
                pz, py, px = prev
                m[(pz + z) // 2, (py + y) // 2, px] = 2
                if pz != z:
                    assert py == y
            m[z, y, :] = 2
            end = W - 1 if forward else 0
            prev = (z, y, end)
            forward = not forward
    return m


def score_of(shape):
    """a non-negative fp32 volume: seeded uniform values, a quarter of them exact zeros, some exact ties"""
    rng = np.random.default_rng(99 + sum(shape))
    s = rng.random(shape, dtype=np.float32)
    s[rng.random(shape) < 0.25] = 0.0
    s[rng.random(shape) < 0.1] = np.float32(0.75)
    return s


@functools.lru_cache(maxsize=None)
def case(shape, kind):
    """the uint8 volume of one of MASKS on one of SHAPES; shared: do not write to it.  The main value is 2, so that
    label = 2 and label = 0 both have something to find."""
    D, H, W = shape
    z = np.zeros(shape, np.uint8)
    ax = int(np.argmax(shape))
    if kind.startswith("rand"):
        rng = np.random.default_rng(31 + sum(shape) + int(kind[4:]))
        fg = rng.random(shape) < int(kind[4:]) / 100.0
        val = np.full(shape, 2, np.uint8)
        if shape == THREE_VALUES:
            val = np.array([2, 1, 3], np.uint8)[np.arange(D) * 3 // D][:, None, None] + z
        return np.where(fg, val, 0).astype(np.uint8)
    if kind == "empty":
        return z
    if kind == "full":
        return z + 2
    if kind == "checker":
        g = np.indices(shape).sum(0)
        return ((g % 2 == 0) * 2).astype(np.uint8)
    if kind == "serpentine":
        return serpentine(shape)
    if kind == "comb":                       # teeth along y on the even (z, x), joined by the slab y = H - 1 alone
        m = z.copy()
        m[::2, :H - 1, ::2] = 2
        m[:, H - 1, :] = 2
        return m
    if kind == "edge_corner":                # pairs that touch across an edge or a corner only, spread along the longest axis
        m = z.copy()
        offs = [(0, 1, 1), (1, 0, 1), (1, 1, 0), (1, 1, 1), (0, 1, -1), (1, -1, 1), (1, 1, -1), (1, 0, -1), (1, -1, 0), (0, 0, 1)]
        for k, off in enumerate(offs):
            base = [1 if o < 0 else 0 for o in off]
            base[ax] += 4 * k
            q = tuple(b + o for b, o in zip(base, off))
            if _inside(shape, base) and _inside(shape, q):
                m[tuple(base)] = 2
                m[q] = 2
        return m
    if kind == "wrap":                       # the end of a row and the start of the next; the end of a plane and the start of the next
        m = z.copy()
        ya = max(min(2, H - 2), 0)
        m[0, ya, W - 1] = 2
        if H > 1:
            m[0, ya + 1, 0] = 2
        m[0, H - 1, W - 1] = 2
        if D > 1:
            m[1, 0, 0] = 2
        if D > 2 and H > 2:                   # and the same in the middle of the volume
            m[D // 2, H // 2, W - 1] = 2
            m[D // 2, H // 2 + 1 if H // 2 + 1 < H else 0, 0] = 2
        return m
    if kind == "planes2":                    # two values in alternate planes (rows of a depth-1 volume)
        a = 0 if D > 1 else 1
        sh = [1, 1, 1]
        sh[a] = shape[a]
        alt = np.where(np.arange(shape[a]) % 2 == 0, 2, 5).astype(np.uint8).reshape(sh)
        return (alt + z).astype(np.uint8)
    if kind == "tie":                        # along the longest axis: value 2 in pieces of 2, 2, 1 voxels, value 3 in 1, 2, 2
        m = z.copy()
        line = np.zeros(shape[ax], np.uint8)
        for lo, hi, v in ((0, 2, 2), (5, 7, 2), (10, 11, 2), (14, 15, 3), (18, 20, 3), (23, 25, 3)):
            line[lo:hi] = v                   # (cut off where the axis is shorter)
        sl = [0, 0, 0]
        sl[ax] = slice(None)
        m[tuple(sl)] = line
        return m
    raise KeyError(kind)


def case_ref(shape, kind, connectivity, lab):
    """(not cached: eight filtered maps a call, and every test asks for its own)"""
    return full(case(shape, kind), connectivity, lab, score_of(shape))
