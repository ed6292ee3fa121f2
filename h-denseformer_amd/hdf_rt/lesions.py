"""Lesion-wise matching on the device: the overlap table of two labelings and the two per-lesion protocols built on it --
detection matching (PI-CAI style: a predicted lesion is a hit when it overlaps a ground-truth lesion enough, its
confidence is the peak probability inside it) and the BraTS-2023 lesion-wise Dice and HD95.  What a user does today with two
copies of int32 id maps to the host (2 x 470 MB for a 448x512x512 volume) and np.unique over 64-bit keys on one thread.  Every
function labels, dilates and joins on the device and makes ONE copy to the host, of a table of a few thousand words.
The lesion-wise HD95 (lesion_wise_scores(hd95=True): per kept truth lesion `surface`, `hd` and `hd95`, at the top
`lesion_hd95`, a missed lesion and a false positive scoring `hd95_penalty`) carves every lesion's box out of the id maps
and runs the surface entry on the crops (hdf_lesion_surface); it makes a second copy, of twelve words a lesion.
Kernels: csrc/cc_pairs.hip, csrc/lesion_surface.hip (and components.hip, morphology.hip, surface.hip); definitions:
include/hdf.h.  No CPU fallback.

connectivity, label and the numbering of the components are those of hdf_rt.components: ids 1..n in ascending order of
each component's smallest linear voxel index.  A [H, W] input is the depth-1 volume [1, H, W]."""
import ctypes
import struct

import torch

from . import _lib
from ._lib import check, lib, ptr, stream_ptr
from ._volume import WorkspaceCache, as_volume, clear_all
from .components import _label, component_table
from .morphology import binary_dilation
from .surface import _spacing, scores_from_result, scores_from_result_mm

PAIRS_A0, PAIRS_B0 = 1, 2            # HDF_PAIRS_*
PAIR_COLS = ("a", "b", "n", "m")
# one workspace per capacity and stream (_volume.WorkspaceCache): 256 + 24 bytes a table slot (a power of two >=
# 2 * capacity), in a cache of its own
_workspaces = WorkspaceCache("hdf_cc_pairs_workspace_bytes")


def clear_workspaces():
    """drop the cached workspaces: these, and those of the other entries on a volume (as hdf_rt.surface's)"""
    clear_all()


def _volume(a, what):
    """a uint8 or bool map as components takes it: (uint8 [D][H][W] on the GPU, the caller's shape)"""
    return as_volume(a, what, dtypes=(torch.uint8, torch.bool), who="connected components need")


def _ids(t, what):
    if not (torch.is_tensor(t) and t.dtype == torch.int32 and t.device.type == "cuda" and t.dim() in (2, 3)):
        raise ValueError(f"{what} must be an int32 device tensor [D, H, W] or [H, W]")
    t = t.contiguous()
    return t[None] if t.dim() == 2 else t


def component_overlap(ids_a, ids_b, mask=None, capacity=4096, zero_a=False, zero_b=False):
    """(pairs int64 [capacity, 4], result int64 [4]) on the device; nothing waits on the host.  pairs: one row a, b, n, m
    (PAIR_COLS) per distinct pair of ids that share a voxel, in ascending (a, b): n voxels, m of them where `mask` (uint8
    or bool, same shape; None: m = 0) is non-zero; zeros behind the last pair.  Counted: a > 0 and b > 0; with zero_a also
    a == 0 and b > 0, with zero_b also a > 0 and b == 0 -- with both, a component's size is the sum of its rows.  An id
    below 0 counts as 0.  result: pairs, counted voxels, counted voxels under the mask, overflow (more distinct pairs than
    `capacity`: everything else is then 0).  ids_a, ids_b: int32 device tensors, e.g. from connected_components."""
    if not torch.cuda.is_available():
        raise _lib.HdfError("component overlap needs a GPU (there is no CPU path)")
    a, b = _ids(ids_a, "ids_a"), _ids(ids_b, "ids_b")
    if a.shape != b.shape or a.device != b.device:
        raise ValueError(f"ids_a {tuple(ids_a.shape)} and ids_b {tuple(ids_b.shape)} must match, on one device")
    shape = tuple(int(s) for s in a.shape)
    if mask is not None:
        mask, _ = _volume(mask, "mask")
        if tuple(mask.shape) != shape or mask.device != a.device:
            raise ValueError(f"mask {tuple(mask.shape)} does not match the id maps {shape}")
    capacity = int(capacity)
    flags = (PAIRS_A0 if zero_a else 0) | (PAIRS_B0 if zero_b else 0)
    with torch.cuda.device(a.device):
        ws = _workspaces.workspace(a.device, capacity)
        pairs = torch.empty((capacity, 4), dtype=torch.int64, device=a.device)
        res = torch.empty(4, dtype=torch.int64, device=a.device)
        check(lib().hdf_cc_pairs(ptr(a), ptr(b), ptr(mask), flags, *shape, capacity, ptr(pairs), ptr(res), ptr(ws), ws.numel(),
                                 stream_ptr()), "hdf_cc_pairs")
    return pairs, res


def _rows(host, what, capacity):
    """the rows of a table copied to the host as a flat list: result[4], then pairs"""
    if host[3]:
        raise _lib.HdfError(f"{what}: more than {capacity} distinct pairs, capacity {capacity}")
    return [host[4 + 4 * i: 8 + 4 * i] for i in range(host[0])]


def overlap_value(n, size_a, size_b, overlap):
    if overlap == "dice":
        return 2.0 * n / (size_a + size_b)
    return n / (size_a + size_b - n)          # 'iou', and the order under 'any'


def _match_rows(rows, n_pred, n_truth, min_overlap, overlap):
    """The host half of the detection matching, shared by match_components and detection.match_candidates: from the rows
    (a, b, n, m) of an overlap table with both zero flags, the sizes, the candidate pairs and the greedy one-to-one
    assignment.  The result dict of match_components with confidence = None."""
    size_p, size_t = [0] * (n_pred + 1), [0] * (n_truth + 1)
    for a, b, n, _m in rows:
        size_p[a] += n
        size_t[b] += n
    cand = []
    for a, b, n, _m in rows:
        if a > 0 and b > 0:
            ov = overlap_value(n, size_p[a], size_t[b], overlap)
            if overlap == "any" or ov >= min_overlap:
                cand.append((-ov, b, a))
    cand.sort()
    pred_match, truth_match = [(0, 0.0)] * n_pred, [(0, 0.0)] * n_truth
    for neg, b, a in cand:
        if pred_match[a - 1][0] == 0 and truth_match[b - 1][0] == 0:
            pred_match[a - 1], truth_match[b - 1] = (b, -neg), (a, -neg)
    tp = sum(1 for t, _ in pred_match if t)
    return dict(tp=tp, fp=n_pred - tp, fn=n_truth - tp, truth_match=truth_match, pred_match=pred_match, pred_size=size_p[1:],
                truth_size=size_t[1:], confidence=None)


def match_components(pred, truth, connectivity=26, pred_label=0, truth_label=0, score=None, min_overlap=0.1, overlap="iou",
                     capacity=4096):
    """Detection matching of the components of `pred` (predicted lesions) with those of `truth`, both uint8 / bool maps:
    label both, one overlap table with both zero flags (a component's size is the sum of its rows), with `score` (fp32,
    non-negative, e.g. a class probability) the peak score per predicted lesion, ONE copy to the host.  The peak score is
    hdf_cc_table's score_max: that entry fills its [capacity, 9] table as well, which is not used here.

    A candidate is a pair (a, b) of a predicted and a truth lesion that share n >= 1 voxels and whose overlap is at least
    min_overlap: 'iou' = n / (|A| + |B| - n), 'dice' = 2 n / (|A| + |B|); under 'any' every touching pair is a candidate
    whatever min_overlap is, and its overlap is reported and ordered as the IoU.  The assignment is one-to-one and greedy in
    descending overlap (compared as fp64 values); ties go to the smaller truth id, then to the smaller predicted id.

    Returns a dict: tp, fp, fn; truth_match = per truth lesion (predicted id or 0, overlap); pred_match = per predicted
    lesion (truth id or 0, overlap); pred_size, truth_size; confidence = the score maximum per predicted lesion, or None.
    zip(confidence, (t > 0 for t, _ in pred_match)) are the (confidence, is_tp) records an AP / FROC aggregator takes."""
    if overlap not in ("iou", "dice", "any"):
        raise ValueError(f"overlap must be 'iou', 'dice' or 'any', got {overlap!r}")
    pv, _ = _volume(pred, "pred")
    tv, _ = _volume(truth, "truth")
    if pv.shape != tv.shape:
        raise ValueError(f"pred {tuple(pv.shape)} and truth {tuple(tv.shape)} must match")
    tv = tv.to(pv.device)
    capacity = int(capacity)
    ids_p, res_p = _label(pv, connectivity, pred_label)
    ids_t, res_t = _label(tv, connectivity, truth_label)
    pairs, res = component_overlap(ids_p, ids_t, None, capacity, True, True)
    parts = [res, pairs.reshape(-1), res_p, res_t]
    if score is not None:
        # (every predicted lesion has a row of the pair table: a call that does not overflow has at most `capacity` of them)
        _, smax = component_table(pv, ids_p, score, capacity)
        parts.append(smax.view(torch.int32).to(torch.int64))
    host = torch.cat(parts).cpu().tolist()              # the one D2H copy
    rows = _rows(host, "match_components", capacity)
    tail = 4 + 4 * capacity
    n_pred, n_truth = host[tail], host[tail + 2]
    out = _match_rows(rows, n_pred, n_truth, min_overlap, overlap)
    conf = None
    if score is not None:
        conf = [struct.unpack("<f", struct.pack("<i", w))[0] for w in host[tail + 4: tail + 4 + n_pred]]
    out["confidence"] = conf
    return out


def _lesion_surfaces(ids_p, ids_t, g, pairs, n_pairs, boxes, spacing):
    """hdf_lesion_surface for the rows `boxes` = [(j, zmin, zmax, ymin, ymax, xmin, xmax)]: the result rows as lists of twelve
    ints, after ONE copy to the host.  One allocation of the size the entry asks for; it is not kept."""
    shape = tuple(int(s) for s in ids_p.shape)
    L = len(boxes)
    rows7 = (ctypes.c_int32 * (7 * L))(*[int(v) for row in boxes for v in row])
    sp = None if spacing is None else _spacing(spacing)
    with torch.cuda.device(ids_p.device):
        need = lib().hdf_lesion_surface_workspace_bytes(rows7, L, *shape, 0 if sp is None else 1)
        if need < 0:
            raise _lib.HdfError("hdf_lesion_surface_workspace_bytes: " + lib().hdf_last_error().decode(errors="replace"))
        ws = torch.empty(need, dtype=torch.uint8, device=ids_p.device)
        results = torch.empty((L, 12), dtype=torch.int64, device=ids_p.device)
        check(lib().hdf_lesion_surface(ptr(ids_p), ptr(ids_t), ptr(g), *shape, ptr(pairs), n_pairs, rows7, L, sp, ptr(ws),
                                       ws.numel(), ptr(results), stream_ptr()), "hdf_lesion_surface")
        return results.cpu().tolist()          # the second and last D2H copy


def lesion_wise_scores(pred, truth, label, dilate_iterations=3, dilate_connectivity=18, connectivity=26, min_size=0,
                       capacity=4096, hd95=False, spacing=None, hd95_penalty=374.0):
    """The BraTS-2023 lesion-wise Dice of class `label` (1..255), and with hd95=True its lesion-wise HD95.  G = truth == label; Gd = G dilated dilate_iterations
    times under dilate_connectivity (hdf_rt.binary_dilation; 0 iterations: Gd = G); the truth lesions are the components of
    Gd, the predicted lesions those of pred == label, both under `connectivity`.  One overlap table with mask = G and both
    zero flags, ONE copy to the host.  For truth lesion j:
      gt_j   = the voxels of G inside it                  P_j = the predicted lesions that share a voxel with it
      tp_j   = the voxels of G inside it that P_j covers  dice_j = 2 tp_j / (the voxels of P_j + gt_j)
    A truth lesion with gt_j < min_size is dropped (it neither scores nor counts).  A predicted lesion in no P_j -- of the
    dropped lesions too -- is a false positive.  lesion_dice = sum of dice_j / (kept truth lesions + false positives), 1.0
    when there is neither.  All in fp64.

    Returns a dict: lesions = per kept truth lesion a dict (id, gt, tp, pred = the ids of P_j, pred_voxels, dice),
    dropped = the ids of the dropped truth lesions, false_positives = the predicted ids in no P_j, fp, lesion_dice.

    hd95=False is exactly that: the same dict from the same launches and the same single copy.  hd95=True adds the
    protocol's second number.  The two component tables (hdf_cc_table) join the one copy; the box of lesion j is the union
    of the box of truth lesion j and of the boxes of P_j; then ONE hdf_lesion_surface call for the kept lesions with a
    non-empty P_j -- the masks (gt_j, P_j) carved on their boxes grown by one voxel, hdf_surface_distances on every crop --
    and a second and last copy, of its twelve words a lesion.  The crop is exact: every seed, contour voxel and neighbour of
    a mask voxel lies inside it, a clamped side is the volume's face, an unclamped one is true background, and a mask fills
    the crop only if it fills the volume -- the words are those of the full-volume call.  spacing: None (voxels) or
    (sz, sy, sx) as hdf_rt.surface takes it (hdf_surface_distances_mm); without hd95=True it is a ValueError.
    Every kept lesion's dict gains surface (the twelve ints), hd and hd95 (surface.scores_from_result / _mm: the Hausdorff
    distance and its 95th percentile, in voxels or in the spacing's unit).  A kept lesion with an empty P_j has surface =
    None and hd = hd95 = hd95_penalty.  A lesion whose masks the surface entry calls invalid (gt_j or P_j fills the
    volume) has hd = hd95 = NaN in its own dict and counts as hd95_penalty in the aggregate.  The top level gains
    lesion_hd95 = (the sum of hd95 over the kept lesions + hd95_penalty * fp) / (kept truth lesions + fp), 0.0 when there
    is neither.  All in fp64.  surface[0] and surface[1] must equal gt and pred_voxels of the overlap table: an HdfError
    names the lesion where they do not (a box that did not contain its lesion)."""
    label, capacity, iters = int(label), int(capacity), int(dilate_iterations)
    if not 1 <= label <= 255:
        raise ValueError(f"label must be in 1..255, got {label}")
    if spacing is not None:
        if not hd95:
            raise ValueError("spacing is the unit of the lesion-wise HD95: pass hd95=True with it")
        _spacing(spacing)
    penalty = float(hd95_penalty)
    pv, _ = _volume(pred, "pred")
    tv, _ = _volume(truth, "truth")
    if pv.shape != tv.shape:
        raise ValueError(f"pred {tuple(pv.shape)} and truth {tuple(tv.shape)} must match")
    tv = tv.to(pv.device)
    g = (tv == label).to(torch.uint8)
    gd = binary_dilation(g, dilate_connectivity, iters) if iters > 0 else g
    ids_p, res_p = _label(pv, connectivity, label)
    ids_t, res_t = _label(gd, connectivity, 0)
    pairs, res = component_overlap(ids_p, ids_t, g, capacity, True, True)
    parts = [res, pairs.reshape(-1), res_p, res_t]
    if hd95:
        parts += [component_table(pv, ids_p, None, capacity).reshape(-1), component_table(gd, ids_t, None, capacity).reshape(-1)]
    host = torch.cat(parts).cpu().tolist()          # the one D2H copy (with hd95: the first of two)
    rows = _rows(host, "lesion_wise_scores", capacity)
    tail = 4 + 4 * capacity
    n_pred, n_truth = host[tail], host[tail + 2]
    size_p = [0] * (n_pred + 1)
    gt, tp, touching = [0] * (n_truth + 1), [0] * (n_truth + 1), [[] for _ in range(n_truth + 1)]
    for a, b, n, m in rows:                 # ascending (a, b): every list of P_j comes out in ascending a
        size_p[a] += n
        gt[b] += m
        if a > 0 and b > 0:
            tp[b] += m
            touching[b].append(a)
    matched = set()
    lesions, dropped, total = [], [], 0.0
    for j in range(1, n_truth + 1):
        matched.update(touching[j])
        if gt[j] < min_size:
            dropped.append(j)
            continue
        vox = sum(size_p[a] for a in touching[j])
        dice = 2.0 * tp[j] / (vox + gt[j])
        total += dice
        lesions.append(dict(id=j, gt=gt[j], tp=tp[j], pred=touching[j], pred_voxels=vox, dice=dice))
    false_pos = [a for a in range(1, n_pred + 1) if a not in matched]
    denom = len(lesions) + len(false_pos)
    out = dict(lesions=lesions, dropped=dropped, false_positives=false_pos, fp=len(false_pos),
               lesion_dice=total / denom if denom else 1.0)
    if not hd95:
        return out

    def box(base, i):        # row i - 1 of a component table: zmin, zmax, ymin, ymax, xmin, xmax
        return host[base + 9 * (i - 1) + 3: base + 9 * (i - 1) + 9]

    tab_p = tail + 4
    tab_t = tab_p + 9 * capacity
    scored = [les for les in lesions if les["pred"]]
    boxes = []
    for les in scored:
        bs = [box(tab_t, les["id"])] + [box(tab_p, a) for a in les["pred"]]
        boxes.append([les["id"]] + [f(b[k] for b in bs) for k, f in enumerate((min, max) * 3)])
    words = _lesion_surfaces(ids_p, ids_t, g, pairs, host[0], boxes, spacing) if scored else []
    for les, row in zip(scored, words):
        if (row[0], row[1]) != (les["gt"], les["pred_voxels"]):
            raise _lib.HdfError(f"lesion_wise_scores: lesion {les['id']}: its crop holds {row[0]} truth and {row[1]} predicted "
                                f"voxels, the overlap table {les['gt']} and {les['pred_voxels']}")
        s = scores_from_result(row) if spacing is None else scores_from_result_mm(row)
        les.update(surface=row, hd=s["HausdorffDistance"], hd95=s["HausdorffDistance95"])
    total_hd = 0.0
    for les in lesions:
        if not les["pred"]:
            les.update(surface=None, hd=penalty, hd95=penalty)
        total_hd += penalty if les["hd95"] != les["hd95"] else les["hd95"]          # (NaN: an invalid pair of masks)
    out["lesion_hd95"] = (total_hd + penalty * len(false_pos)) / denom if denom else 0.0
    return out
