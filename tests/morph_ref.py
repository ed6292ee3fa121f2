"""The morphology definitions of include/hdf.h restated in numpy (no GPU part), the inputs and the case list of the GPU
test, the one comparison both the GPU test and the planted-defect test use, and the planted defects.

A step is a shifted OR (dilate) or AND (erode) over the offsets (dz, dy, dx) in {-1, 0, 1}^3 with |dz| + |dy| + |dx| <= c
(c = 1 / 2 / 3 for connectivity 6 / 18 / 26) of the mask padded by one voxel of border_value; a depth-1 volume has no z
offsets and no z padding.  OPEN is n erosions then n dilations, CLOSE n dilations then n erosions.  Fill holes labels the
complement with scipy.ndimage.label and fills the components that touch no face (no edge, at depth 1).  tests/
test_morph_ref_cpu.py holds all of this to scipy's own binary_* functions."""
import functools
import itertools

import numpy as np
from scipy import ndimage as ndi

CONNECTIVITIES = (6, 18, 26)
C_OF = {6: 1, 18: 2, 26: 3}
DILATE, ERODE, OPEN, CLOSE = 0, 1, 2, 3          # HDF_MORPH_*
OPS = (DILATE, ERODE, OPEN, CLOSE)
OP_NAMES = {DILATE: "dilate", ERODE: "erode", OPEN: "open", CLOSE: "close"}
MASK, MAP = 0, 1
STRUCTURE = {c: ndi.generate_binary_structure(3, C_OF[c]) for c in CONNECTIVITIES}

# the planted defects (test_morph_ref_cpu.py): each is a way the kernels could be wrong that the comparison must notice
DEFECTS = ("c18_as_26", "border_ignored", "one_iteration_short", "carry_across_rows", "tail_bits_zero", "flat_z_border",
           "face_hole_filled", "other_class_overwritten")


def in_mask(vol, label):
    return vol == label if label else vol != 0


def offsets(connectivity, flat):
    c = C_OF[connectivity]
    return [(dz, dy, dx) for dz, dy, dx in itertools.product((-1, 0, 1), repeat=3)
            if abs(dz) + abs(dy) + abs(dx) <= c and not (flat and dz)]


def step(mask, connectivity, border_value, erode, defect=None):
    """one dilation or erosion of a bool [D, H, W] mask"""
    D, H, W = mask.shape
    flat = D == 1 and defect != "flat_z_border"
    if defect == "c18_as_26" and connectivity == 18:
        connectivity = 26
    if defect == "border_ignored":
        border_value = 0
    pad = np.full((D + 2, H + 2, W + 2), bool(border_value))
    pad[1:-1, 1:-1, 1:-1] = mask
    if defect == "carry_across_rows":       # what lies past a row's end is the next row's first voxel, in linear order
        rows = mask.reshape(D * H, W)
        right = np.append(rows[1:, 0], bool(border_value))
        left = np.insert(rows[:-1, -1], 0, bool(border_value))
        pad[1:-1, 1:-1, -1] = right.reshape(D, H)
        pad[1:-1, 1:-1, 0] = left.reshape(D, H)
    if defect == "tail_bits_zero" and W % 32:   # the bits of the last word past W, read as they were packed: 0
        pad[1:-1, 1:-1, -1] = False
    acc = np.full(mask.shape, bool(erode))
    for dz, dy, dx in offsets(connectivity, flat):
        sh = pad[1 + dz: 1 + dz + D, 1 + dy: 1 + dy + H, 1 + dx: 1 + dx + W]
        acc = (acc & sh) if erode else (acc | sh)
    return acc


def write_out(vol, label, old, new, mode, defect=None):
    """(out uint8, [voxels of the new mask, voxels where the masks differ])"""
    res = [int(np.count_nonzero(new)), int(np.count_nonzero(new ^ old))]
    if mode == MASK:
        return new.astype(np.uint8), res
    assert label >= 1
    out = vol.copy()
    out[old & ~new] = 0
    joined = new & ~old
    out[joined if defect == "other_class_overwritten" else joined & (vol == 0)] = label
    return out, res


def morph(vol, label, op, connectivity, iterations, border_value, mode, defect=None):
    assert iterations >= 1 and vol.ndim == 3
    old = in_mask(vol, label)
    n = iterations - 1 if defect == "one_iteration_short" else iterations
    m = old
    for erode in {DILATE: (0,), ERODE: (1,), OPEN: (1, 0), CLOSE: (0, 1)}[op]:
        for _ in range(n):
            m = step(m, connectivity, border_value, erode, defect)
    return write_out(vol, label, old, m, mode, defect)


def fill_holes(vol, label, connectivity, mode, defect=None):
    old = in_mask(vol, label)
    lab, n = ndi.label(~old, STRUCTURE[connectivity])
    faces = [lab[:, 0], lab[:, -1], lab[:, :, 0]]
    if defect != "face_hole_filled":
        faces.append(lab[:, :, -1])
    if vol.shape[0] > 1:                       # a depth-1 volume has edges only
        faces += [lab[0], lab[-1]]
    outside = np.zeros(n + 1, bool)
    for f in faces:
        outside[f.ravel()] = True
    outside[0] = True                          # (id 0 is the mask itself)
    new = old | ~outside[lab]
    return write_out(vol, label, old, new, mode, defect)


def mismatches(got, want):
    """names of what differs between two (out, result) pairs -- every byte and both result words compared exactly; the
    comparison of the GPU test, and the one the planted defects must not get past"""
    bad = []
    a, b = np.asarray(got[0]), np.asarray(want[0])
    if a.dtype != np.uint8 or a.shape != b.shape or not np.array_equal(a, b):
        bad.append("out")
    if [int(v) for v in got[1]] != [int(v) for v in want[1]]:
        bad.append("result")
    return bad


# ------------------------------------------------------------------------------------------------------ inputs
SHAPES = ([(1, 1, 1), (1, 37, 70)] + [(4, 5, w) for w in (31, 32, 33, 63, 64, 65)] +
          [(3, 5, 48), (5, 3, 300), (19, 67, 131), (1024, 2, 3), (2, 1024, 3), (3, 2, 1024), (40, 48, 56)])
MASKS = ["rand20", "rand50", "rand80", "rand97", "empty", "full", "corners_centre", "checker", "wrap", "box", "box_gap",
         "hole_face", "nested", "contact"]
THREE_VALUES = (40, 48, 56)       # the shape whose random fills carry three values, in slabs along z
ITERATIONS = (1, 2, 3, 17)
MODE_LABEL = ((MASK, 0), (MASK, 2), (MAP, 2))


def _walls(shape):
    """per axis (a, b): the box has walls at a and b and its inside between them -- one voxel off the faces where the axis
    has five voxels or more, on the faces where it has three or four, and no wall (None) on a shorter axis"""
    return [(1, s - 2) if s >= 5 else (0, s - 1) if s >= 3 else None for s in shape]


def _box(shape):
    m = np.zeros(shape, np.uint8)
    w = _walls(shape)
    outer = tuple(slice(None) if r is None else slice(r[0], r[1] + 1) for r in w)
    inner = tuple(slice(None) if r is None else slice(r[0] + 1, r[1]) for r in w)
    m[outer] = 2
    m[inner] = 0
    return m, w, inner


@functools.lru_cache(maxsize=None)
def case(shape, kind):
    """the uint8 volume of one of MASKS on one of SHAPES; shared: do not write to it.  The main value is 2, so that
    label = 2 and label = 0 both have something to find."""
    D, H, W = shape
    z = np.zeros(shape, np.uint8)
    if kind.startswith("rand"):
        rng = np.random.default_rng(57 + sum(shape) + int(kind[4:]))
        fg = rng.random(shape) < int(kind[4:]) / 100.0
        val = np.full(shape, 2, np.uint8)
        if shape == THREE_VALUES:
            val = np.array([2, 1, 3], np.uint8)[np.arange(D) * 3 // D][:, None, None] + z
        return np.where(fg, val, 0).astype(np.uint8)
    if kind == "empty":
        return z
    if kind == "full":
        return z + 2
    if kind == "corners_centre":
        m = z.copy()
        for p in itertools.product(*[(0, s - 1) for s in shape]):
            m[p] = 2
        m[D // 2, H // 2, W // 2] = 2
        return m
    if kind == "checker":
        return ((np.indices(shape).sum(0) % 2 == 0) * 2).astype(np.uint8)
    if kind == "wrap":                       # the last column of a row and the first of the next row (and of the next plane)
        m = z.copy()
        ya = max(min(2, H - 2), 0)
        m[D // 2, ya, W - 1] = 2
        if H > 1:
            m[D // 2, ya + 1, 0] = 2
        m[0, H - 1, W - 1] = 2
        if D > 1:
            m[1, 0, 0] = 2
        return m
    if kind == "box":                        # one hole
        return _box(shape)[0]
    if kind == "box_gap":
        # the x = b wall two voxels thick, less one voxel of its inner layer and the voxel of its outer layer one row on: the
        # two touch across an edge only, so the hole is closed for a 6-connected background and open for 18 / 26
        m, w, _ = _box(shape)
        if w[2] is not None and w[1] is not None and w[2][1] - w[2][0] >= 4 and w[1][1] - w[1][0] >= 2:
            b = w[2][1]
            zs = slice(None) if w[0] is None else slice(w[0][0], w[0][1] + 1)
            ys = slice(w[1][0], w[1][1] + 1)
            m[zs, ys, b - 1] = 2
            zc, yc = D // 2, w[1][0] + 1
            m[zc, yc, b - 1] = 0
            m[zc, yc + 1, b] = 0
        return m
    if kind == "hole_face":                  # the box open towards x = 0: its hole touches that face
        m, w, inner = _box(shape)
        if w[2] is not None:
            m[inner[0], inner[1], : w[2][0] + 1] = 0
        return m
    if kind == "nested":                     # an object inside the hole, a second box inside where there is room
        m, w, inner = _box(shape)
        m[D // 2, H // 2, W // 2] = 2
        if all(r is not None and r[1] - r[0] >= 6 for r in w):
            core = tuple(slice(r[0] + 2, r[1] - 1) for r in w)
            hollow = tuple(slice(r[0] + 3, r[1] - 2) for r in w)
            m[core] = 2
            m[hollow] = 0
        return m
    if kind == "contact":                    # two classes in contact along the longest axis, background on both sides
        m = z.copy()
        ax = int(np.argmax(shape))
        s = shape[ax]
        line = np.zeros(s, np.uint8)
        line[s // 4: s // 2] = 2
        line[s // 2: 3 * s // 4] = 1
        sh = [1, 1, 1]
        sh[ax] = s
        return (m + line.reshape(sh)).astype(np.uint8)
    raise KeyError(kind)


_COMBOS = list(itertools.product(CONNECTIVITIES, OPS, (0, 1), ITERATIONS, MODE_LABEL))      # 288


@functools.lru_cache(maxsize=None)
def morph_params(index, per_case=36):
    """the (connectivity, op, border_value, iterations, mode, label) sets that case number `index` of SHAPES x MASKS runs:
    thirty-six of the 288 combinations, taken in a fixed scattered order (101 is prime to 288: a permutation).  The
    fourteen masks of a shape are consecutive cases and take 504 consecutive places of that order, so every shape runs
    every combination, and every (shape, mask) pair the three connectivities"""
    out = []
    for k in range(per_case):
        c, op, bv, n, (mode, label) = _COMBOS[(index * per_case + k) * 101 % len(_COMBOS)]
        out.append((c, op, bv, n, mode, label))
    return out


FILL_PARAMS = [(c, mode, label) for c in CONNECTIVITIES for mode, label in MODE_LABEL]
CASES = [(s, k) for s in SHAPES for k in MASKS]


def refusals(vol, out, res, ws, ws_bytes, fill_ws_bytes, shape=(4, 5, 6)):
    """(what, entry, arguments) of every refusal include/hdf.h lists; vol / out / res / ws are addresses that a refused
    call never dereferences.  test_morph_ref_cpu.py passes host addresses,
    test_gpu_morphology.py device memory that it checks afterwards."""
    D, H, W = shape
    V = D * H * W

    def m(label=0, op=DILATE, conn=6, n=1, bv=0, mode=MASK, dims=shape, vol=vol, out=out, res=res, ws=ws, nb=ws_bytes):
        return "hdf_morph", (vol, label, op, conn, n, bv, mode) + tuple(dims) + (out, res, ws, nb, None)

    def f(label=0, conn=6, mode=MASK, dims=shape, vol=vol, out=out, res=res, ws=ws, nb=fill_ws_bytes):
        return "hdf_fill_holes", (vol, label, conn, mode) + tuple(dims) + (out, res, ws, nb, None)

    cases = []
    for both, kw in [("a dimension of 0", dict(dims=(0, H, W))), ("a dimension of 1025", dict(dims=(D, H, 1025))),
                     ("a negative dimension", dict(dims=(D, -3, W))), ("connectivity 8", dict(conn=8)),
                     ("connectivity 0", dict(conn=0)), ("label -1", dict(label=-1)), ("label 256", dict(label=256)),
                     ("mode 2", dict(mode=2)), ("mode -1", dict(mode=-1)), ("MAP with label 0", dict(mode=MAP, label=0)),
                     ("null volume", dict(vol=None)), ("null out", dict(out=None)), ("null result", dict(res=None)),
                     ("null workspace", dict(ws=None)), ("workspace not aligned", dict(ws=ws + 4)),
                     ("out overlaps volume", dict(out=vol + 8)), ("out overlaps volume from below", dict(vol=out + V - 1)),
                     ("workspace overlaps volume", dict(vol=ws + 16)), ("workspace overlaps out", dict(out=ws + 8))]:
        cases.append((both, ) + m(**kw))
        cases.append((both, ) + f(**kw))
    cases.append(("workspace one byte short", ) + m(nb=ws_bytes - 1))
    cases.append(("workspace one byte short", ) + f(nb=fill_ws_bytes - 1))
    cases.append(("workspace of the other entry", ) + f(nb=ws_bytes))
    for what, kw in [("iterations 0", dict(n=0)), ("iterations -1", dict(n=-1)), ("iterations 257", dict(n=257)),
                     ("border_value 2", dict(bv=2)), ("border_value -1", dict(bv=-1)), ("op 4", dict(op=4)),
                     ("op -1", dict(op=-1))]:
        cases.append((what, ) + m(**kw))
    return cases
