"""The lesion-wise HD95 of hdf_rt.lesion_wise_scores(hd95=True) and the result rows of hdf_lesion_surface (include/hdf.h)
restated with numpy / scipy (no GPU part), the inputs of the GPU tests and the comparison both test files use.

lesion_hd_ref extends lesion_ref.lesion_wise_ref: per kept truth lesion it builds the two FULL-VOLUME boolean masks (gt_j,
P_j) and hands them to surface_ref.surface / surface_mm_ref.surface.  It crops nothing, so a device result that equals it
also proves the crop.  `crop` and `defect` are for tests/test_lesion_hd_ref_cpu.py: the same masks evaluated on a box, and
deliberately wrong readings of the protocol."""
import functools
import struct

import numpy as np
from scipy import ndimage as ndi

import cc_ref as cr
import lesion_ref as lr
import surface_mm_ref as smr
import surface_ref as sr

DEFECTS = ("tight_crop", "dilated_truth", "no_pool", "all_pred", "miss_scores_zero", "fp_unpenalised")
SPACING = (2.5, 0.8, 1.1)
PENALTY = 374.0


def crop_box(mask, margin=1):
    """slices of the bounding box of a non-empty boolean mask, grown by `margin` voxels and clamped to the volume"""
    idx = np.nonzero(mask)
    return tuple(slice(max(int(i.min()) - margin, 0), min(int(i.max()) + margin, s - 1) + 1) for i, s in zip(idx, mask.shape))


def surface_words(T, P, spacing=None, box=None):
    """result[12] of the surface restatement for two boolean masks, on the whole volume or on the slices `box`"""
    if box is not None:
        T, P = T[box], P[box]
    t, p = np.ascontiguousarray(T, np.uint8), np.ascontiguousarray(P, np.uint8)
    if spacing is None:
        return [int(v) for v in sr.surface(t, p, 1)["result"]]
    return [int(v) for v in smr.surface(t, p, 1, tuple(spacing))["result"]]


def lesion_masks(pred, truth, label, dilate_iterations=3, dilate_connectivity=18, connectivity=26, defect=None):
    """(G, lab_p, n_pred, lab_t, n_truth, [(j, T_j, touching ids, P_j)]) from scipy's labelling; T_j, P_j boolean volumes"""
    pred, truth = np.asarray(pred), np.asarray(truth)
    if pred.ndim == 2:
        pred, truth = pred[None], truth[None]
    G = truth == label
    Gd = ndi.binary_dilation(G, cr.STRUCTURE[dilate_connectivity], dilate_iterations) if dilate_iterations > 0 else G
    lab_t, n_truth = ndi.label(Gd, cr.STRUCTURE[connectivity])
    lab_p, n_pred = ndi.label(pred == label, cr.STRUCTURE[connectivity])
    out = []
    for j in range(1, n_truth + 1):
        bj = lab_t == j
        touching = sorted(int(i) for i in np.unique(lab_p[bj]) if i)
        T = bj if defect == "dilated_truth" else G & bj
        pool = touching
        if defect == "no_pool" and touching:
            pool = [max(touching, key=lambda i: (int((lab_p == i).sum()), -i))]
        P = np.isin(lab_p, pool) if pool else np.zeros(G.shape, bool)
        if defect == "all_pred" and touching:
            P = lab_p > 0
        out.append((j, T, touching, P))
    return G, lab_p, n_pred, lab_t, n_truth, out


def lesion_hd_ref(pred, truth, label, dilate_iterations=3, dilate_connectivity=18, connectivity=26, min_size=0, spacing=None,
                  hd95_penalty=PENALTY, defect=None, crop=None):
    """the dict of hdf_rt.lesion_wise_scores(..., hd95=True).  crop: None (full-volume masks), or the margin of the box of
    gt_j and P_j the surface restatement is evaluated on instead (1: what the device does, 0: the planted tight_crop)"""
    assert defect is None or defect in DEFECTS
    out = lr.lesion_wise_ref(pred, truth, label, dilate_iterations, dilate_connectivity, connectivity, min_size)
    _, _, _, _, _, masks = lesion_masks(pred, truth, label, dilate_iterations, dilate_connectivity, connectivity, defect)
    if defect == "tight_crop":
        crop = 0
    by_id = {j: (T, P) for j, T, _touching, P in masks}
    penalty = float(hd95_penalty)
    total = 0.0
    for les in out["lesions"]:
        T, P = by_id[les["id"]]
        if not les["pred"]:
            miss = 0.0 if defect == "miss_scores_zero" else penalty
            les.update(surface=None, hd=miss, hd95=miss)
        else:
            words = surface_words(T, P, spacing, None if crop is None else crop_box(T | P, crop))
            s = sr.scores(words) if spacing is None else smr.scores(words)
            les.update(surface=words, hd=s["HausdorffDistance"], hd95=s["HausdorffDistance95"])
        total += penalty if les["hd95"] != les["hd95"] else les["hd95"]
    fp = 0 if defect == "fp_unpenalised" else out["fp"]
    denom = len(out["lesions"]) + out["fp"]
    out["lesion_hd95"] = (total + penalty * fp) / denom if denom else 0.0
    return out


def entry_inputs(pred, truth, label, dilate_iterations=3, dilate_connectivity=18, connectivity=26, capacity=4096, **_unused):
    """what hdf_lesion_surface takes for one case, from scipy alone: ids_pred, ids_truth int32, the mask G uint8, the pair rows
    (lesion_ref.pairs_ref, both zero flags) and their number, lesions int32 [L][7] = every truth lesion with a non-empty P_j
    and the tight box of gt_j and P_j, and the full-volume masks [(T_j, P_j)] in that order"""
    G, lab_p, _n_pred, lab_t, _n_truth, masks = lesion_masks(pred, truth, label, dilate_iterations, dilate_connectivity,
                                                             connectivity)
    pairs, res = lr.pairs_ref(lab_p, lab_t, G, lr.A0 | lr.B0, capacity)
    assert res[3] == 0
    rows, full = [], []
    for j, T, touching, P in masks:
        if not touching:
            continue
        box = crop_box(T | P, 0)
        rows.append([j] + [v for s in box for v in (s.start, s.stop - 1)])
        full.append((T, P))
    return dict(ids_pred=lab_p.astype(np.int32), ids_truth=lab_t.astype(np.int32), mask=G.astype(np.uint8), pairs=pairs,
                n_pairs=res[0], lesions=np.asarray(rows, np.int32).reshape(-1, 7), masks=full)


def crop_layout(lesions, shape):
    """[(offset of the truth crop, crop slices)] of the workspace of hdf_lesion_surface as include/hdf.h lays it out: crops from
    byte 0 in row order, 2 bytes a crop voxel, the truth mask first"""
    out, at = [], 0
    for row in np.asarray(lesions).reshape(-1, 7):
        box = tuple(slice(max(int(row[1 + 2 * k]) - 1, 0), min(int(row[2 + 2 * k]) + 1, shape[k] - 1) + 1) for k in range(3))
        out.append((at, box))
        at += 2 * int(np.prod([s.stop - s.start for s in box]))
    return out, at


def _bits(x):
    return struct.pack("<d", x) if isinstance(x, float) else x


def mismatches(got, want):
    """paths of what differs between two result dicts: ints, lists and None compared exactly, floats in every bit (NaN equals
    the NaN of the same bits) -- the comparison of the GPU test, and the one the planted defects must not get past"""
    bad = []

    def walk(a, b, path):
        if isinstance(a, dict) and isinstance(b, dict):
            if list(a.keys()) != list(b.keys()):
                bad.append(path + ".keys")
                return
            for k in a:
                walk(a[k], b[k], f"{path}.{k}")
        elif isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)):
            if len(a) != len(b):
                bad.append(path + ".len")
                return
            for i, (x, y) in enumerate(zip(a, b)):
                walk(x, y, f"{path}[{i}]")
        elif type(a) is not type(b) or _bits(a) != _bits(b):
            bad.append(path)

    walk(got, want, "")
    return bad


# ------------------------------------------------------------------------------------------------------ inputs
# (1,1,1): a mask that fills the volume; (8,8,70): a crop row longer than a wave; (17,16,65), (24,40,48): several workgroups
SHAPES = [(1, 1, 1), (1, 9, 33), (5, 6, 7), (3, 17, 33), (8, 8, 70), (17, 16, 65), (24, 40, 48)]
SEEDS = (0, 1, 2, 3)
LATTICE_SHAPE = (24, 40, 48)


def _boxes(shape, *boxes):
    m = np.zeros(shape, np.uint8)
    for z0, z1, y0, y1, x0, x1 in boxes:
        m[z0:z1, y0:y1, x0:x1] = 1
    return m


@functools.lru_cache(maxsize=None)
def hand_cases():
    """{name: (pred, truth, kwargs of lesion_wise_scores)}; shared: do not write to the arrays"""
    s = (7, 11, 19)
    out = {}
    # a lesion in the corner (0, 0, 0): three sides of its crop are clamped
    out["corner"] = (_boxes(s, (0, 2, 0, 3, 1, 3)), _boxes(s, (0, 2, 0, 2, 0, 2)), dict(dilate_iterations=1))
    # a predicted bar across two truth lesions: one predicted id in two P_j, two crops that overlap
    out["bar"] = (_boxes(s, (3, 4, 5, 6, 2, 16)), _boxes(s, (2, 5, 4, 7, 1, 4), (3, 5, 5, 8, 13, 16)), dict(dilate_iterations=1))
    # a truth lesion nothing touches, a lone false positive, and a matched pair between them
    out["miss_and_fp"] = (_boxes(s, (0, 2, 8, 10, 15, 18), (4, 6, 4, 6, 8, 11)),
                          _boxes(s, (5, 7, 0, 2, 0, 3), (4, 6, 4, 7, 7, 10)), dict(dilate_iterations=1))
    # the same maps undilated: P_j needs a shared voxel
    out["no_dilation"] = out["bar"][:2] + (dict(dilate_iterations=0),)
    # a one-voxel truth lesion below min_size: dropped, its predicted neighbour counts as matched (no false positive)
    out["min_size"] = (_boxes(s, (1, 2, 1, 2, 2, 3), (4, 6, 4, 6, 8, 11)), _boxes(s, (1, 2, 1, 2, 1, 2), (4, 6, 4, 7, 7, 10)),
                       dict(dilate_iterations=1, min_size=2))
    # the truth fills the volume: the surface entry calls the masks invalid (NaN in the lesion, the penalty in the aggregate)
    out["full_truth"] = (_boxes((3, 4, 5), (1, 2, 1, 3, 1, 4)), np.ones((3, 4, 5), np.uint8), dict(dilate_iterations=1))
    # a lesion as long as the volume: crop rows of 69 voxels, longer than a wave and no multiple of anything
    out["long_row"] = (_boxes((3, 5, 69), (1, 2, 1, 4, 0, 69)), _boxes((3, 5, 69), (0, 2, 2, 3, 3, 66)), dict(dilate_iterations=1))
    # only false positives, only misses, nothing at all
    out["only_fp"] = (out["miss_and_fp"][0], np.zeros(s, np.uint8), {})
    out["only_miss"] = (np.zeros(s, np.uint8), out["miss_and_fp"][1], {})
    out["nothing"] = (np.zeros(s, np.uint8), np.zeros(s, np.uint8), {})
    # 100 one-voxel truth lesions, each with a one-voxel prediction two voxels along x: more lesions than one carve launch
    # takes (64).  The tight box of gt_j and P_j is 1 x 1 x 3, its crop 3 x 3 x 5 (7 x 7 x 7 from the dilated lesion's box):
    # odd width, odd size, so every predicted crop starts at an odd byte
    truth, pred = np.zeros(LATTICE_SHAPE, np.uint8), np.zeros(LATTICE_SHAPE, np.uint8)
    for z in (2, 8, 14, 20):
        for y in (3, 11, 19, 27, 35):
            for x in (4, 14, 24, 34, 44):
                truth[z, y, x], pred[z, y, x + 2] = 1, 1
    out["lattice"] = (pred, truth, dict(dilate_iterations=2))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    """[(name, pred, truth, label, kwargs)]: lesion_ref.blob_pair with seeds 0..3 on every shape, then the hand-made ones"""
    out = []
    for shape in SHAPES:
        for seed in SEEDS:
            pred, truth, _score = lr.blob_pair(shape, seed)
            out.append(("x".join(map(str, shape)) + f"-s{seed}", pred, truth, 1, {}))
    out[0] = (out[0][0], np.ones((1, 1, 1), np.uint8), np.ones((1, 1, 1), np.uint8), 1, {})   # (1,1,1): both masks full
    for name, (pred, truth, kw) in hand_cases().items():
        out.append((name, pred, truth, 1, kw))
    return out


CASE_NAMES = [c[0] for c in cases()]


def case(name):
    return cases()[CASE_NAMES.index(name)]


@functools.lru_cache(maxsize=None)
def case_ref(name, spacing=None):
    """lesion_hd_ref of one case; shared: do not write to it"""
    _name, pred, truth, label, kw = case(name)
    return lesion_hd_ref(pred, truth, label, spacing=spacing, **kw)


@functools.lru_cache(maxsize=None)
def case_entry(name):
    _name, pred, truth, label, kw = case(name)
    return entry_inputs(pred, truth, label, **kw)


@functools.lru_cache(maxsize=None)
def case_entry_words(name, spacing=None):
    """the result rows hdf_lesion_surface must leave for case_entry(name): the restatement on the full-volume masks"""
    return [surface_words(T, P, spacing) for T, P in case_entry(name)["masks"]]
