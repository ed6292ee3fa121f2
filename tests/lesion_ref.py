"""The overlap table of two id maps (include/hdf.h, hdf_cc_pairs) and the two lesion-wise protocols of hdf_rt.lesions
restated with numpy / scipy (no GPU part), the inputs of the GPU tests and the one comparison both the GPU test and the
planted-defect test use.

pairs_ref is np.unique over 64-bit keys.  match_ref and lesion_wise_ref are NOT built on it: they work from per-lesion
boolean masks (scipy.ndimage.label and binary_dilation on the masks, set arithmetic per lesion), so that the protocols
are checked independently of the table."""
import functools
import os
import re

import numpy as np
from scipy import ndimage as ndi

import cc_ref as cr

A0, B0 = 1, 2            # HDF_PAIRS_*
FLAGS = (0, A0, B0, A0 | B0)


def pairs_ref(ids_a, ids_b, mask=None, flags=0, capacity=4096):
    """(pairs int64 [capacity, 4] = rows a, b, n, m in ascending (a, b), zeros behind them; result = [P, sum n, sum m,
    overflow]).  More than `capacity` distinct pairs: all zeros and the flag."""
    a = np.maximum(np.asarray(ids_a, np.int64).ravel(), 0)
    b = np.maximum(np.asarray(ids_b, np.int64).ravel(), 0)
    counted = (a > 0) & (b > 0)
    if flags & A0:
        counted |= (a == 0) & (b > 0)
    if flags & B0:
        counted |= (a > 0) & (b == 0)
    keys, inverse, n = np.unique((a[counted] << 32) | b[counted], return_inverse=True, return_counts=True)
    m = np.zeros(len(keys), np.int64)
    if mask is not None:
        under = np.asarray(mask).ravel()[counted] != 0
        m = np.bincount(inverse.ravel()[under], minlength=len(keys)).astype(np.int64)
    pairs = np.zeros((capacity, 4), np.int64)
    if len(keys) > capacity:
        return pairs, [0, 0, 0, 1]
    pairs[:len(keys)] = np.stack([keys >> 32, keys & 0xffffffff, n, m], axis=1)
    return pairs, [len(keys), int(n.sum()), int(m.sum()), 0]


def mismatches(got, want):
    """names of what differs between two (pairs, result): every int64 of pairs and every word of result compared exactly --
    the comparison of the GPU test, and the one the planted defects must not get past"""
    bad = []
    gp, wp = np.asarray(got[0], np.int64), np.asarray(want[0], np.int64)
    if gp.shape != wp.shape or not np.array_equal(gp, wp):
        bad.append("pairs")
    if [int(v) for v in got[1]] != [int(v) for v in want[1]]:
        bad.append("result")
    return bad


# ------------------------------------------------------------------------------------------------------ protocols
def overlap_value(n, size_a, size_b, overlap):
    if overlap == "dice":
        return 2.0 * n / (size_a + size_b)
    return n / (size_a + size_b - n)


def match_ref(pred, truth, connectivity=26, pred_label=0, truth_label=0, score=None, min_overlap=0.1, overlap="iou"):
    """detection matching from per-lesion boolean masks: the dict of hdf_rt.match_components"""
    pred, truth = np.asarray(pred, np.uint8), np.asarray(truth, np.uint8)
    if pred.ndim == 2:
        pred, truth = pred[None], truth[None]
        score = None if score is None else np.asarray(score)[None]
    ids_p, n_pred = cr.label(pred, connectivity, pred_label)
    ids_t, n_truth = cr.label(truth, connectivity, truth_label)
    A = [ids_p == i for i in range(1, n_pred + 1)]
    B = [ids_t == j for j in range(1, n_truth + 1)]
    size_p, size_t = [int(x.sum()) for x in A], [int(x.sum()) for x in B]
    cand = []
    for j, bj in enumerate(B, 1):
        for i in np.unique(ids_p[bj]):
            if i == 0:
                continue
            n = int((A[i - 1] & bj).sum())
            ov = overlap_value(n, size_p[i - 1], size_t[j - 1], overlap)
            if overlap == "any" or ov >= min_overlap:
                cand.append((ov, j, int(i)))
    pred_match, truth_match = [(0, 0.0)] * n_pred, [(0, 0.0)] * n_truth
    # descending overlap; a tie to the smaller truth id, then to the smaller predicted id
    for ov, j, i in sorted(cand, key=lambda c: (-c[0], c[1], c[2])):
        if pred_match[i - 1][0] == 0 and truth_match[j - 1][0] == 0:
            pred_match[i - 1], truth_match[j - 1] = (j, ov), (i, ov)
    tp = sum(1 for t, _ in pred_match if t)
    conf = None
    if score is not None:
        s = np.asarray(score, np.float32).reshape(pred.shape)
        conf = [np.float32(s[x].max()) for x in A]
    return dict(tp=tp, fp=n_pred - tp, fn=n_truth - tp, truth_match=truth_match, pred_match=pred_match, pred_size=size_p,
                truth_size=size_t, confidence=conf)


def lesion_wise_ref(pred, truth, label, dilate_iterations=3, dilate_connectivity=18, connectivity=26, min_size=0):
    """the BraTS-2023 lesion-wise Dice from per-lesion boolean masks: the dict of hdf_rt.lesion_wise_scores"""
    pred, truth = np.asarray(pred), np.asarray(truth)
    if pred.ndim == 2:
        pred, truth = pred[None], truth[None]
    G = truth == label
    Gd = ndi.binary_dilation(G, cr.STRUCTURE[dilate_connectivity], dilate_iterations) if dilate_iterations > 0 else G
    lab_t, n_truth = ndi.label(Gd, cr.STRUCTURE[connectivity])
    lab_p, n_pred = ndi.label(pred == label, cr.STRUCTURE[connectivity])
    lesions, dropped, matched, total = [], [], set(), 0.0
    for j in range(1, n_truth + 1):
        bj = lab_t == j
        touching = sorted(int(i) for i in np.unique(lab_p[bj]) if i)
        matched.update(touching)
        gt = int((G & bj).sum())
        if gt < min_size:
            dropped.append(j)
            continue
        pm = np.isin(lab_p, touching) if touching else np.zeros(pred.shape, bool)
        tp, vox = int((G & bj & pm).sum()), int(pm.sum())
        dice = 2.0 * tp / (vox + gt)
        total += dice
        lesions.append(dict(id=j, gt=gt, tp=tp, pred=touching, pred_voxels=vox, dice=dice))
    false_pos = [i for i in range(1, n_pred + 1) if i not in matched]
    denom = len(lesions) + len(false_pos)
    return dict(lesions=lesions, dropped=dropped, false_positives=false_pos, fp=len(false_pos),
                lesion_dice=total / denom if denom else 1.0)


# ------------------------------------------------------------------------------------------------------ inputs
def geometry():
    """TRIP, SPAN, LDS_SLOTS, SORT_CHUNK, MAX_CAPACITY of the kernels, read from csrc/cc_pairs.h (its constants are integer
    expressions of one another)"""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "h-denseformer_amd", "csrc", "cc_pairs.h")
    out = {}
    for name, expr in re.findall(r"constexpr \w+ HDF_PAIRS_([A-Z_]+) = ([^;]+);", open(path).read()):
        assert re.fullmatch(r"[A-Z_0-9 *+]+", expr), expr
        out[name] = int(eval(re.sub(r"HDF_PAIRS_([A-Z_]+)", lambda m: str(out[m.group(1)]), expr), {}))
    return out


# (8,32,32) is one workgroup's span exactly, (1,9,911) leaves the second workgroup seven voxels, (5,29,113) the third one
SHAPES = [(1, 1, 1), (1, 1, 63), (1, 1, 64), (1, 1, 65), (1, 3, 70), (2, 5, 37), (1, 40, 40), (3, 17, 33), (9, 20, 257),
          (24, 40, 48), (8, 32, 32), (1, 9, 911), (5, 29, 113)]
MAPS = ["empty", "a_empty", "b_empty", "one_pair", "blobs", "synthetic", "same", "negative"]
MASKS = [None, "random", "zeros", "all255"]
SORT_SHAPE = (24, 40, 48)       # with the synthetic maps: more pairs than one workgroup sorts


def blobs(shape, seed, count, rmax=5.0, value=1):
    """a uint8 map with `count` seeded ellipsoids of `value` (some may merge or fall partly outside)"""
    rng = np.random.default_rng(seed)
    grid = np.indices(shape).astype(np.float64)
    out = np.zeros(shape, np.uint8)
    for _ in range(count):
        c = [rng.uniform(0, s) for s in shape]
        r = [max(rng.uniform(1.0, rmax), 0.6) for _ in shape]
        out[sum(((grid[k] - c[k]) / r[k]) ** 2 for k in range(len(shape))) <= 1.0] = value
    return out


@functools.lru_cache(maxsize=None)
def blob_pair(shape, seed, value=1):
    """(pred, truth, score): a truth map of seeded blobs and a prediction that keeps most of them displaced or resized, misses
    some, splits some and adds some of its own; score: a non-negative fp32 volume.  Shared: do not write to them."""
    rng = np.random.default_rng(1000 + seed)
    grid = np.indices(shape).astype(np.float64)
    truth, pred = np.zeros(shape, np.uint8), np.zeros(shape, np.uint8)

    def ball(c, r):
        return sum(((grid[k] - c[k]) / r[k]) ** 2 for k in range(len(shape))) <= 1.0

    for _ in range(int(rng.integers(3, 12))):
        c = [rng.uniform(0, s) for s in shape]
        r = [rng.uniform(1.0, 4.5) for _ in shape]
        truth[ball(c, r)] = value
        kind = rng.random()
        if kind < 0.2:
            continue                                              # missed
        shift = [rng.uniform(-2.0, 2.0) for _ in shape]
        scale = rng.uniform(0.5, 1.4)
        hit = ball([a + b for a, b in zip(c, shift)], [scale * v for v in r])
        if kind > 0.8 and shape[-1] > 4:                          # split by a cut through its centre
            cut = min(max(int(c[-1]), 0), shape[-1] - 1)
            hit[..., cut] = False
        pred[hit] = value
    for _ in range(int(rng.integers(0, 4))):                      # spurious
        pred[ball([rng.uniform(0, s) for s in shape], [rng.uniform(0.8, 2.5) for _ in shape])] = value
    score = rng.random(shape, dtype=np.float32)
    score[rng.random(shape) < 0.2] = np.float32(0.5)
    return pred, truth, score


@functools.lru_cache(maxsize=None)
def id_maps(shape, kind):
    """(ids_a, ids_b) int32 for one of MAPS but 'blobs' (whose ids come from hdf_cc_label in the GPU test and from
    cc_ref.label here); shared: do not write to them"""
    v = np.arange(int(np.prod(shape)), dtype=np.int64).reshape(shape)
    z = np.zeros(shape, np.int32)
    if kind == "empty":
        return z, z.copy()
    if kind == "a_empty":
        return z, (1 + v // 7).astype(np.int32)
    if kind == "b_empty":
        return (1 + v // 7).astype(np.int32), z
    if kind == "one_pair":
        return z + 3, z + 70000
    if kind == "synthetic":              # many pairs, the same pair on both sides of every row start
        return (1 + v // 3).astype(np.int32), (1 + v // 5).astype(np.int32)
    if kind == "same":
        a = (v // 11 % 5).astype(np.int32)
        return a, a
    if kind == "negative":
        rng = np.random.default_rng(7 + sum(shape))
        a = rng.integers(-3, 4, shape).astype(np.int32)
        b = rng.integers(-2, 3, shape).astype(np.int32)
        return a, b
    if kind == "blobs":
        a = cr.label(blobs(shape, 11 + sum(shape), 9), 26)[0]
        b = cr.label(blobs(shape, 12 + sum(shape), 9), 26)[0]
        return a, b
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def mask_of(shape, kind):
    if kind is None:
        return None
    if kind == "zeros":
        return np.zeros(shape, np.uint8)
    if kind == "all255":
        return np.full(shape, 255, np.uint8)
    rng = np.random.default_rng(5 + sum(shape))
    return (rng.integers(0, 3, shape) * 100).astype(np.uint8)       # 0, 100, 200
