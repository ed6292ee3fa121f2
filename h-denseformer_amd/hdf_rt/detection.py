"""Detection evaluation on the device: lesion candidates from a probability map, their matching with the truth lesions, and
the aggregator that turns matched cases into AP, AUROC and FROC -- the ranking of a detection challenge such as PI-CAI,
which the 2-D model's workload is.  What a user does today with a copy of the fp32 map to the host (470 MB for 448x512x512)
and one scipy.ndimage.label per round.  slice_predict(..., return_probabilities=True)[1] goes through
extract_lesion_candidates and match_candidates into DetectionEvaluator with one small copy to the host per stage.
Kernels: csrc/detect.hip (and components.hip, cc_pairs.hip); the protocol: include/hdf.h.  No CPU fallback for the two
device functions; DetectionEvaluator is host code and needs no GPU.

The protocol follows the "dynamic" lesion extraction of PI-CAI evaluation (peak, threshold at peak / 2.5, the component
of the peak, drop candidates adjacent to an accepted one, five lesions) as include/hdf.h states it; it was not compared
with that package.  A [H, W] input is the depth-1 volume [1, H, W]."""
import struct

import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr, stream_ptr
from ._volume import WorkspaceCache, clear_all
from .lesions import _ids, _match_rows, _rows, _volume, component_overlap
from .components import _label

TABLE_COLS = ("index", "m_bits", "size", "peak", "status", "thr_bits")
STATUS = ("kept", "adjacent", "small")
FINISHED = {1: "count", 2: "stop"}
# one workspace per volume shape and stream (_volume.WorkspaceCache), about 14 bytes a voxel, in a cache of its own
_workspaces = WorkspaceCache("hdf_detect_workspace_bytes")


def clear_workspaces():
    """drop the cached workspaces: these, and those of the other entries on a volume (as hdf_rt.surface's)"""
    clear_all()


def _f32(bits):
    return struct.unpack("<f", struct.pack("<I", bits))[0]


def _f64(bits):
    return struct.unpack("<d", struct.pack("<q", bits))[0]


def candidates_from_rows(rows):
    """the table rows (six ints each, TABLE_COLS) as the list of dicts extract_lesion_candidates returns"""
    return [dict(index=r[0], confidence=_f32(r[1]), size=r[2], peak=r[3], status=STATUS[r[4]], threshold=_f64(r[5]))
            for r in rows]


def _extract(prob, num_lesions, factor, stop, connectivity, remove_adjacent, min_voxels, max_rounds, sync_every,
             table_rows=None):
    """extract_lesion_candidates with the table's length free: (detection_map, indexed, rows, result words, copies)"""
    if not torch.cuda.is_available():
        raise _lib.HdfError("lesion candidates need a GPU (there is no CPU path)")
    if not torch.is_tensor(prob):
        prob = torch.from_numpy(np.ascontiguousarray(prob))
    if prob.dim() not in (2, 3) or prob.dtype != torch.float32:
        raise ValueError(f"prob must be fp32 [D, H, W] or [H, W], got {prob.dtype} {tuple(prob.shape)}")
    max_rounds, sync_every = int(max_rounds), int(sync_every)
    if max_rounds < 1 or sync_every < 1:
        raise ValueError(f"max_rounds {max_rounds} and sync_every {sync_every} must be at least 1")
    shape = tuple(prob.shape)
    p = prob.to("cuda").contiguous() if prob.device.type != "cuda" else prob.contiguous()
    p = p[None] if p.dim() == 2 else p
    dims = tuple(int(s) for s in p.shape)
    table_rows = max_rounds if table_rows is None else int(table_rows)
    with torch.cuda.device(p.device):
        ws = _workspaces.workspace(p.device, *dims)
        det = torch.empty(dims, dtype=torch.float32, device=p.device)
        idx = torch.empty(dims, dtype=torch.int32, device=p.device)
        table = torch.empty((table_rows, 6), dtype=torch.int64, device=p.device)
        res = torch.empty(4, dtype=torch.int64, device=p.device)
        done, copies = 0, 0
        while True:
            n = min(sync_every, max_rounds - done)
            check(lib().hdf_detect_candidates(ptr(p), *dims, int(num_lesions), float(factor), float(stop), int(connectivity),
                                              int(bool(remove_adjacent)), int(min_voxels), done, n, ptr(det), ptr(idx),
                                              ptr(table) if table_rows else None, table_rows, ptr(res), ptr(ws), ws.numel(),
                                              stream_ptr()), "hdf_detect_candidates")
            words = res.cpu().tolist()                       # the four result words: the one copy of a chunk
            copies += 1
            if words[2] == 3:
                raise _lib.HdfError(f"hdf_detect_candidates: the state stands at another round than {done}")
            done = words[0]
            if words[2] != 0 or done >= max_rounds:
                break
        rows = table[:min(done, table_rows)].cpu().tolist()  # and one more for the table
    return det.view(shape), idx.view(shape), rows, words, copies + 1


def extract_lesion_candidates(prob, num_lesions=5, threshold_factor=2.5, stop_threshold=0.01, connectivity=6,
                              remove_adjacent=True, min_voxels=0, max_rounds=256, sync_every=8):
    """Lesion candidates of a fp32 probability map (a device tensor, or a numpy array that is uploaded once), by the
    protocol of include/hdf.h: per round the peak m at its first index a, the mask prob > m / threshold_factor (fp64), the
    component of a under `connectivity` (6 / 18 / 26, scipy's generate_binary_structure(3, 1 / 2 / 3)); the candidate is
    dropped as 'adjacent' when remove_adjacent and it touches (26-neighbourhood) an accepted one, else as 'small' below
    min_voxels, else kept: its voxels get the confidence m in detection_map and the next index in `indexed`.  Every
    candidate leaves the working copy.  The loop ends with num_lesions kept ('count'), with a peak below stop_threshold
    ('stop'), or after max_rounds rounds ('rounds').

    The entry runs in chunks of sync_every rounds; after each chunk the four result words are copied to the host, and at
    the end the table: 1 + ceil(rounds / sync_every) small copies, nothing else leaves the device.  Rounds of a chunk
    behind the finish run their launches on an empty mask and change nothing.

    Returns a dict: detection_map (fp32 device tensor shaped like prob), indexed (int32 device tensor), candidates = one
    dict per round in order (index = 1.. for a kept one and 0 for a dropped one, confidence, size, peak = the linear index
    of a, status = 'kept' | 'adjacent' | 'small', threshold), rounds, finished."""
    det, idx, rows, words, _ = _extract(prob, num_lesions, threshold_factor, stop_threshold, connectivity, remove_adjacent,
                                        min_voxels, max_rounds, sync_every)
    return dict(detection_map=det, indexed=idx, candidates=candidates_from_rows(rows), rounds=words[0],
                finished=FINISHED.get(words[2], "rounds"))


def match_candidates(indexed, truth, candidates=None, connectivity=26, truth_label=0, min_overlap=0.1, overlap="iou",
                     capacity=4096):
    """match_components for the candidates of extract_lesion_candidates: the predicted lesions are the ids of `indexed`
    itself (int32 device tensor), not relabelled -- two candidates that touch stay two -- and the truth lesions the
    components of `truth` (uint8 / bool) under `connectivity`.  One overlap table with both zero flags, ONE copy to the
    host.  candidates: the list extract_lesion_candidates returned; the number of predicted lesions is then its kept
    candidates and confidence[i - 1] the confidence of the one with index i.  Without it the number is the largest id that
    has a voxel, and confidence is None.  Returns the dict of match_components."""
    if overlap not in ("iou", "dice", "any"):
        raise ValueError(f"overlap must be 'iou', 'dice' or 'any', got {overlap!r}")
    tv, _ = _volume(truth, "truth")
    ids_p = _ids(indexed, "indexed")
    if ids_p.shape != tv.shape:
        raise ValueError(f"indexed {tuple(ids_p.shape)} and truth {tuple(tv.shape)} must match")
    tv = tv.to(ids_p.device)
    capacity = int(capacity)
    ids_t, res_t = _label(tv, connectivity, truth_label)
    pairs, res = component_overlap(ids_p, ids_t, None, capacity, True, True)
    host = torch.cat([res, pairs.reshape(-1), res_t]).cpu().tolist()          # the one D2H copy
    rows = _rows(host, "match_candidates", capacity)
    return _match_candidate_rows(rows, host[4 + 4 * capacity], candidates, min_overlap, overlap)


def _match_candidate_rows(rows, n_truth, candidates, min_overlap, overlap):
    """the host half of match_candidates: lesions._match_rows with the predicted ids and confidences of the candidates"""
    conf = None
    if candidates is None:
        n_pred = max((a for a, _b, _n, _m in rows), default=0)
    else:
        kept = sorted((c["index"], c["confidence"]) for c in candidates if c["index"] > 0)
        if [i for i, _ in kept] != list(range(1, len(kept) + 1)):
            raise ValueError("candidates: the indices of the kept candidates must be 1..n")
        n_pred, conf = len(kept), [c for _, c in kept]
        if any(a > n_pred for a, _b, _n, _m in rows):
            raise ValueError(f"indexed holds an id above the {n_pred} kept candidates")
    out = _match_rows(rows, n_pred, n_truth, min_overlap, overlap)
    out["confidence"] = conf
    return out


class DetectionEvaluator:
    """Collects matched cases and aggregates them (host only).  A lesion record is (confidence, is_tp): one per predicted
    lesion, and (0.0, True) per missed truth lesion -- it is found only at threshold 0, where everything is positive.  A case
    record is (score, label): the highest confidence of the case, or 0.

    ap()     step-wise average precision over the lesion records: sum over the distinct confidences t, descending, of
             (R_t - R_prev) * P_t, records of equal confidence entering together.  NaN without a positive record.
    auroc()  the Mann-Whitney statistic over the case records, ties counted 1/2.  NaN when one class is absent.
    froc()   at every distinct confidence t of a predicted lesion, descending: the sensitivity (true positives with
             confidence >= t over all truth lesions) and the false positives (>= t) per case.
    score()  (ap + auroc) / 2."""

    def __init__(self):
        self.lesions = []   # (confidence, is_tp): the predicted lesions and the missed truth lesions
        self.predicted = []  # (confidence, is_tp): the predicted lesions alone
        self.cases = []     # (score, label)
        self.n_truth = 0
        self.n_pred = 0

    def add_case(self, match, case_label=None):
        """match: the dict of match_candidates / match_components, with its confidence list"""
        conf = match["confidence"]
        if conf is None:
            raise ValueError("the match has no confidences: pass candidates= (or score=) to the matching")
        pred, truth = match["pred_match"], match["truth_match"]
        if len(conf) != len(pred):
            raise ValueError(f"{len(conf)} confidences for {len(pred)} predicted lesions")
        for c, (t, _ov) in zip(conf, pred):
            self.lesions.append((float(c), t > 0))
            self.predicted.append((float(c), t > 0))
        self.n_pred += len(pred)
        for a, _ov in truth:
            if a == 0:
                self.lesions.append((0.0, True))
        self.n_truth += len(truth)
        label = len(truth) > 0 if case_label is None else bool(case_label)
        self.cases.append((max([float(c) for c in conf], default=0.0), label))

    def ap(self):
        pos = sum(1 for _, tp in self.lesions if tp)
        if pos == 0:
            return float("nan")
        recs = sorted(self.lesions, key=lambda r: -r[0])
        ap, tp, n, prev_recall, i = 0.0, 0, 0, 0.0, 0
        while i < len(recs):
            j = i
            while j < len(recs) and recs[j][0] == recs[i][0]:
                tp += recs[j][1]
                j += 1
            n, i = j, j
            recall = tp / pos
            ap += (recall - prev_recall) * (tp / n)
            prev_recall = recall
        return ap

    def auroc(self):
        pos = [s for s, lab in self.cases if lab]
        neg = [s for s, lab in self.cases if not lab]
        if not pos or not neg:
            return float("nan")
        wins = sum((p > q) + 0.5 * (p == q) for p in pos for q in neg)
        return wins / (len(pos) * len(neg))

    def froc(self):
        """dict: thresholds (descending), sensitivity, fp_per_case -- three lists of one length"""
        preds = sorted(self.predicted, key=lambda r: -r[0])
        thresholds, sens, fpc = [], [], []
        tp = fp = i = 0
        while i < len(preds):
            j = i
            while j < len(preds) and preds[j][0] == preds[i][0]:
                tp += preds[j][1]
                fp += not preds[j][1]
                j += 1
            thresholds.append(preds[i][0])
            sens.append(tp / self.n_truth if self.n_truth else float("nan"))
            fpc.append(fp / len(self.cases))
            i = j
        return dict(thresholds=thresholds, sensitivity=sens, fp_per_case=fpc)

    def score(self):
        return (self.ap() + self.auroc()) / 2
