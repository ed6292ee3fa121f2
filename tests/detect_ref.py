"""The numpy restatement of the lesion-candidate protocol of include/hdf.h (hdf_detect_candidates), with a flood fill of
its own, the inputs and parameter sets that the CPU and the GPU tests share, and the matching of candidates from
per-lesion boolean masks.  tests/test_detect_ref_cpu.py holds the restatement to a literal scipy loop in every output bit
and shows that six planted defects are caught; tests/test_gpu_detect.py holds the device to the restatement.

extract_ref returns (det fp32, idx int32, table int64 [rounds][6], finished) with the table rows (index, bits of m, size,
a, status, fp64 bits of thr) and finished in 'count' | 'stop' | 'rounds'."""
import functools

import numpy as np

FLT_MAX = np.finfo(np.float32).max
DEFECTS = ("last_index", "fp32_threshold", "greater_equal", "adjacency_by_connectivity", "dropped_stays", "dropped_takes_index")


def offsets(connectivity):
    """the (dz, dy, dx) != 0 with at most 1 / 2 / 3 non-zero coordinates"""
    nz = {6: 1, 18: 2, 26: 3}[connectivity]
    return [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
            if 0 < abs(dz) + abs(dy) + abs(dx) <= nz]


def flood(mask, seed, connectivity):
    """the boolean map of the component of the linear index `seed` in `mask`: frontier by frontier"""
    D, H, W = mask.shape
    seen = np.zeros(mask.shape, bool)
    flat = seen.reshape(-1)
    flat[seed] = True
    front = np.array([seed], np.int64)
    offs = offsets(connectivity)
    while front.size:
        z, y, x = front // (H * W), front // W % H, front % W
        nxt = []
        for dz, dy, dx in offs:
            zz, yy, xx = z + dz, y + dy, x + dx
            ok = (zz >= 0) & (zz < D) & (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
            n = (zz[ok] * H + yy[ok]) * W + xx[ok]
            n = n[mask.reshape(-1)[n] & ~flat[n]]
            flat[n] = True
            nxt.append(n)
        front = np.unique(np.concatenate(nxt))
    return seen


def touches(cur, taken, connectivity=26):
    """some voxel of `cur` has a voxel of `taken` in its neighbourhood (itself included), clipped at the faces"""
    if (cur & taken).any():
        return True
    D, H, W = cur.shape
    z, y, x = np.nonzero(cur)
    for dz, dy, dx in offsets(connectivity):
        zz, yy, xx = z + dz, y + dy, x + dx
        ok = (zz >= 0) & (zz < D) & (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        if taken[zz[ok], yy[ok], xx[ok]].any():
            return True
    return False


def extract_ref(p, num_lesions=5, factor=2.5, stop=0.01, connectivity=6, remove_adjacent=True, min_voxels=0, max_rounds=256,
                defect=None):
    assert defect is None or defect in DEFECTS
    p = np.asarray(p, np.float32)
    p = p[None] if p.ndim == 2 else p
    with np.errstate(invalid="ignore"):
        w = np.where((p > 0) & (p <= FLT_MAX), p, np.float32(0)).astype(np.float32)
    det, idx = np.zeros(p.shape, np.float32), np.zeros(p.shape, np.int32)
    kept, rows, finished = 0, [], "rounds"
    factor, stop = np.float64(factor), np.float64(stop)
    for _ in range(max_rounds):
        if kept == num_lesions:
            finished = "count"
            break
        flat = w.reshape(-1)
        m = flat.max()
        a = int(np.flatnonzero(flat == m)[-1 if defect == "last_index" else 0])
        if np.float64(m) < stop:
            finished = "stop"
            break
        if defect == "fp32_threshold":
            thr = np.float64(np.float32(m) / np.float32(factor))
        else:
            thr = np.float64(m) / factor
        mask = (w.astype(np.float64) >= thr) if defect == "greater_equal" else (w.astype(np.float64) > thr)
        cur = flood(mask, a, connectivity)
        size = int(cur.sum())
        touch = touches(cur, idx > 0, connectivity if defect == "adjacency_by_connectivity" else 26)
        status = 1 if (remove_adjacent and touch) else 2 if size < min_voxels else 0
        index = 0
        if status == 0:
            kept += 1
            index = kept
            det[cur], idx[cur] = m, kept
        elif defect == "dropped_takes_index":
            index = kept + 1
        if status == 0 or defect != "dropped_stays":
            w[cur] = 0
        rows.append((index, int(np.float32(m).view(np.uint32)), size, a, status, int(thr.view(np.int64))))
    return det, idx, np.array(rows, np.int64).reshape(-1, 6), finished


def same(got, want):
    """the names of the outputs of two (det, idx, table, finished) that differ in some bit"""
    bad = []
    if not np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)):
        bad.append("detection_map")
    if not np.array_equal(got[1], want[1]):
        bad.append("indexed")
    if got[2].shape != want[2].shape or not np.array_equal(got[2], want[2]):
        bad.append("table")
    if got[3] != want[3]:
        bad.append("finished")
    return bad


# ------------------------------------------------------------------------------------------------------ inputs
# (1,1,65): one voxel more than a wave; (1,40,70): the 2-D case, eleven workgroups; (3,5,257): rows one voxel longer than a
# workgroup; (9,65,31) and (12,24,37): odd rows over many workgroups.  BIG: more voxels than GRID_CAP * 256, the most that
# the voxel passes of csrc/detect.hip cover in one trip of their grid-stride loop.
SHAPES = [(1, 1, 1), (1, 1, 65), (1, 40, 70), (5, 17, 33), (12, 24, 37), (9, 65, 31), (3, 5, 257)]
GRID_CAP = 2048                      # HDF_DETECT_GRID_CAP of csrc/detect.h (checked in test_detect_ref_cpu.py)
BIG = (9, 241, 243)                  # 527 067 voxels > 2048 * 256 = 524 288
KINDS = ["blobs", "zeros", "one_voxel", "plateau", "corner", "split", "specials", "below_stop"]
# num_lesions, factor, connectivity, remove_adjacent, min_voxels: every value of every parameter, every pair of
# (connectivity, remove_adjacent), both factors with both num_lesions and both min_voxels
PARAMS = [(5, 2.5, 6, 1, 0), (5, 2.5, 18, 1, 0), (5, 2.5, 26, 1, 0), (5, 2.5, 6, 0, 0), (5, 2.5, 18, 0, 10), (5, 2.5, 26, 0, 10),
          (1, 2.5, 6, 1, 10), (1, 2.5, 26, 0, 0), (5, 1.0000001, 6, 1, 0), (1, 1.0000001, 26, 0, 0), (5, 1.0000001, 18, 0, 10)]
MAX_ROUNDS = 48                      # of the shared cases: factor 1.0000001 takes a voxel or two a round and runs into it


def _box(shape, lo, size):
    """slices of a box at `lo` of `size`, folded into the volume"""
    sl = []
    for s, a, n in zip(shape, lo, size):
        a = min(a, s - 1)
        sl.append(slice(a, min(a + n, s)))
    return tuple(sl)


@functools.lru_cache(maxsize=None)
def volume(kind, shape, seed=0):
    """the fp32 input of a kind on a shape.  Shared: do not write to it."""
    rng = np.random.default_rng(7 + seed + sum(shape) + 31 * KINDS.index(kind))
    D, H, W = shape
    p = np.zeros(shape, np.float32)
    if kind in ("blobs", "specials"):
        grid = np.indices(shape).astype(np.float64)
        for _ in range(int(rng.integers(3, 8))):
            c = [rng.uniform(0, s) for s in shape]
            r = [rng.uniform(0.8, 3.5) for _ in shape]
            g = rng.uniform(0.3, 0.95) * np.exp(-0.5 * sum(((grid[k] - c[k]) / r[k]) ** 2 for k in range(3)))
            p = np.maximum(p, g.astype(np.float32))
        noise = rng.random(shape) < 0.005
        p[noise] = rng.uniform(0.0, 0.6, int(noise.sum())).astype(np.float32)
        if kind == "specials":
            flat = p.reshape(-1)
            for value in (np.nan, -0.75, -0.0, np.inf, -np.inf):
                flat[rng.integers(0, flat.size, max(flat.size // 40, 1))] = value
    elif kind == "one_voxel":
        p.reshape(-1)[p.size // 2] = 0.8
    elif kind == "plateau":
        # two boxes of the same maximum with a lower rim: the first index lies in the box that comes first
        p[_box(shape, (0, 1, 2), (2, 3, 4))] = 0.5
        p[_box(shape, (D // 2, H // 2, W // 2), (2, 3, 5))] = 0.5
        p[_box(shape, (D // 2, H // 2, W // 2 + 6), (1, 1, 2))] = 0.625     # a higher one, a voxel away from the second
        p[_box(shape, (D // 2, H // 2, W // 2 + 8), (1, 1, 1))] = 0.25      # exactly 0.625 / 2.5: on the threshold, not above
    elif kind == "corner":
        # two boxes that share one corner (an axis of length 1: both lie on it)
        pair = [((slice(0, 1),) * 2 if s == 1 else (slice(max(s // 2 - 2, 0), s // 2), slice(s // 2, min(s // 2 + 2, s))))
                for s in shape]
        p[tuple(a for a, _ in pair)] = 0.9
        p[tuple(b for _, b in pair)] = 0.8
    elif kind == "split":
        y, x = H // 2, W // 2
        p[_box(shape, (D // 2, y, 0), (1, 1, W))] = 0.3                     # a bar along x
        p[_box(shape, (D // 2, max(y - 1, 0), x), (1, 3, 1))] = 0.9         # a blob across it
    elif kind == "below_stop":
        p[_box(shape, (0, 0, 0), (2, 2, 2))] = 0.005
        p.reshape(-1)[-1] = 0.0075
    return p


@functools.lru_cache(maxsize=None)
def big_volume():
    """BIG with the only peak in the last voxel, and a few small boxes before it"""
    p = np.zeros(BIG, np.float32)
    rng = np.random.default_rng(99)
    for k in range(6):
        lo = [int(rng.integers(0, s - 4)) for s in BIG]
        p[_box(BIG, lo, (2, 3, 4))] = 0.2 + 0.1 * k
    p[-1, -2:, -3:] = 0.85
    p.reshape(-1)[-1] = 0.95
    return p


@functools.lru_cache(maxsize=None)
def reference(kind, shape, params, max_rounds=MAX_ROUNDS):
    """extract_ref of a shared case, computed once"""
    n, f, c, ra, mv = params
    p = big_volume() if kind == "big" else volume(kind, shape)
    return extract_ref(p, n, f, 0.01, c, bool(ra), mv, max_rounds)


# ------------------------------------------------------------------------------------------------------ matching
def match_ids_ref(ids_p, n_pred, ids_t, n_truth, min_overlap=0.1, overlap="iou"):
    """detection matching of two id maps from per-lesion boolean masks: the dict of hdf_rt.match_candidates without its
    confidence"""
    A = [ids_p == i for i in range(1, n_pred + 1)]
    B = [ids_t == j for j in range(1, n_truth + 1)]
    size_p, size_t = [int(x.sum()) for x in A], [int(x.sum()) for x in B]
    cand = []
    for j, bj in enumerate(B, 1):
        for i, ai in enumerate(A, 1):
            n = int((ai & bj).sum())
            if n == 0:
                continue
            ov = 2.0 * n / (size_p[i - 1] + size_t[j - 1]) if overlap == "dice" else n / (size_p[i - 1] + size_t[j - 1] - n)
            if overlap == "any" or ov >= min_overlap:
                cand.append((ov, j, i))
    pred_match, truth_match = [(0, 0.0)] * n_pred, [(0, 0.0)] * n_truth
    for ov, j, i in sorted(cand, key=lambda c: (-c[0], c[1], c[2])):
        if pred_match[i - 1][0] == 0 and truth_match[j - 1][0] == 0:
            pred_match[i - 1], truth_match[j - 1] = (j, ov), (i, ov)
    tp = sum(1 for t, _ in pred_match if t)
    return dict(tp=tp, fp=n_pred - tp, fn=n_truth - tp, truth_match=truth_match, pred_match=pred_match, pred_size=size_p,
                truth_size=size_t)
