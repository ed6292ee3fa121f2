"""tests/detect_ref.py, the restatement that tests/test_gpu_detect.py holds the device to, is itself held to a literal scipy
loop (ndimage.label with generate_binary_structure(3, c), binary_dilation(idx > 0, ones 3x3x3)) in every output bit -- det,
idx, the table with the bits of thr, the finished reason -- on the inputs, shapes and parameters of the GPU tests; six planted
defects are each shown to be caught by that comparison.  hdf_rt.DetectionEvaluator is held to brute-force definitions over
all thresholds and, where sklearn is installed, to average_precision_score and roc_auc_score at 1e-12, ties and one-class
cases included.  The host half of match_candidates is held to dicts recorded from match_components' host half, as the parent
commit computed them, on the same overlap table.  No GPU."""
import math
import os
import re

import numpy as np
import pytest
from scipy import ndimage as ndi

import detect_ref as dr
from conftest import PKG


def literal(p, num_lesions, factor, stop, connectivity, remove_adjacent, min_voxels, max_rounds):
    """the loop a user writes on the host today"""
    p = np.asarray(p, np.float32)
    p = p[None] if p.ndim == 2 else p
    structure = ndi.generate_binary_structure(3, {6: 1, 18: 2, 26: 3}[connectivity])
    w = p.copy()
    w[~((p > 0) & (p <= np.finfo(np.float32).max))] = 0
    det, idx = np.zeros(p.shape, np.float32), np.zeros(p.shape, np.int32)
    kept, rows = 0, []
    for _ in range(max_rounds):
        if kept == num_lesions:
            return det, idx, np.array(rows, np.int64).reshape(-1, 6), "count"
        a = int(np.argmax(w))                                     # the first index of the maximum
        m = w.reshape(-1)[a]
        if float(m) < stop:
            return det, idx, np.array(rows, np.int64).reshape(-1, 6), "stop"
        thr = float(m) / float(factor)
        labels, _ = ndi.label(w.astype(np.float64) > thr, structure)
        cur = labels == labels.reshape(-1)[a]
        size = int(np.count_nonzero(cur))
        touch = bool((ndi.binary_dilation(idx > 0, np.ones((3, 3, 3), bool)) & cur).any())
        status = 1 if remove_adjacent and touch else 2 if size < min_voxels else 0
        if status == 0:
            kept += 1
            det[cur], idx[cur] = m, kept
        w[cur] = 0
        rows.append((kept if status == 0 else 0, int(np.float32(m).view(np.uint32)), size, a, status,
                     int(np.float64(thr).view(np.int64))))
    return det, idx, np.array(rows, np.int64).reshape(-1, 6), "rounds"


def _literal(kind, shape, params):
    n, f, c, ra, mv = params
    p = dr.big_volume() if kind == "big" else dr.volume(kind, shape)
    return literal(p, n, f, 0.01, c, bool(ra), mv, dr.MAX_ROUNDS)


@pytest.mark.parametrize("shape", dr.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_the_restatement_is_the_literal_scipy_loop(shape):
    reasons, rounds = set(), []
    for kind in dr.KINDS:
        for params in dr.PARAMS:
            want = _literal(kind, shape, params)
            assert dr.same(dr.reference(kind, shape, params), want) == [], (kind, params)
            reasons.add(want[3])
            rounds.append(len(want[2]))
    if shape != (1, 1, 1):
        assert reasons == {"count", "stop", "rounds"} and max(rounds) == dr.MAX_ROUNDS and min(rounds) == 0


def test_the_restatement_on_the_large_volume():
    assert int(np.prod(dr.BIG)) > dr.GRID_CAP * 256
    src = open(os.path.join(PKG, "csrc", "detect.h")).read()
    assert int(re.search(r"HDF_DETECT_GRID_CAP = (\d+);", src).group(1)) == dr.GRID_CAP
    p = dr.big_volume()
    assert int(np.argmax(p)) == p.size - 1 and np.count_nonzero(p == p.max()) == 1
    for params in (dr.PARAMS[0], dr.PARAMS[5]):
        want = _literal("big", dr.BIG, params)
        assert dr.same(dr.reference("big", dr.BIG, params), want) == [], params
        assert want[2][0][3] == p.size - 1 and len(want[2]) >= 5


def test_what_the_inputs_are_there_for():
    shape = (5, 17, 33)
    # the plateau: the maximum of a round at several voxels of two components, and a voxel exactly on the threshold
    det, idx, table, _ = dr.reference("plateau", shape, (5, 2.5, 6, 1, 0))
    w = dr.volume("plateau", shape).copy()
    w[idx == 1] = 0
    lab, n = ndi.label(w == w.max())
    assert n == 2 and np.count_nonzero(w == w.max()) > 2 and table[1][3] == int(np.flatnonzero(w == w.max())[0])
    on_thr = dr.volume("plateau", shape) == np.float32(0.25)
    assert table[0][5] == int(np.float64(0.25).view(np.int64)) and np.count_nonzero(on_thr) == 1 and not (idx == 1)[on_thr].any()
    # the corner: the second box is adjacent under every connectivity, and one component with the first under 26
    for c, rows in ((6, 2), (18, 2), (26, 1)):
        table = dr.reference("corner", shape, (5, 2.5, c, 1, 0))[2]
        assert len(table) == rows and [r[4] for r in table] == [0, 1][:rows], (c, table)
    assert dr.reference("corner", shape, (5, 2.5, 26, 1, 0))[2][0][2] == 16
    assert [r[4] for r in dr.reference("corner", shape, (5, 2.5, 6, 0, 0))[2]] == [0, 0]
    # the split: the mask of the second round is the bar without the blob, in two pieces
    table = dr.reference("split", shape, (5, 2.5, 6, 0, 0))[2]
    assert [r[2] for r in table] == [3, 16, 16]
    # the specials become zeros, the low peak ends the loop in round 0
    p = dr.volume("specials", shape)
    assert np.isnan(p).any() and np.isinf(p).any() and (p < 0).any() and np.signbit(p[p == 0]).any()
    det = dr.reference("specials", shape, (5, 2.5, 6, 1, 0))[0]
    assert np.isfinite(det).all() and (det >= 0).all()
    assert dr.reference("below_stop", shape, dr.PARAMS[0])[3] == "stop" and dr.volume("below_stop", shape).max() > 0


@pytest.mark.parametrize("defect", dr.DEFECTS)
def test_a_planted_defect_is_caught(defect):
    """the restatement with the defect differs from the literal loop on at least one shared case"""
    caught = []
    for shape in ((5, 17, 33), (1, 40, 70)):
        for kind in ("plateau", "corner", "split", "blobs"):
            for params in dr.PARAMS[:7]:
                n, f, c, ra, mv = params
                bad = dr.extract_ref(dr.volume(kind, shape), n, f, 0.01, c, bool(ra), mv, dr.MAX_ROUNDS, defect=defect)
                diff = dr.same(bad, _literal(kind, shape, params))
                if diff:
                    caught.append((shape, kind, params, diff))
    assert caught, defect
    if defect == "greater_equal":
        assert any(kind == "plateau" and "indexed" in d for _, kind, _, d in caught)
    if defect == "last_index":
        assert any(kind == "plateau" for _, kind, _, _ in caught)
    if defect == "adjacency_by_connectivity":
        assert any(kind == "corner" and params[2] == 6 for _, kind, params, _ in caught)


# ------------------------------------------------------------------------------------------------------ the evaluator
def _match(conf_tp, missed):
    """a match dict with the predicted lesions (confidence, is_tp) and `missed` truth lesions nobody found"""
    pred_match = [((k + 1) if tp else 0, 0.5 if tp else 0.0) for k, (_, tp) in enumerate(conf_tp)]
    truth_match = [(i + 1, 0.5) for i, (_, tp) in enumerate(conf_tp) if tp] + [(0, 0.0)] * missed
    return dict(pred_match=pred_match, truth_match=truth_match, confidence=[c for c, _ in conf_tp])


def _brute_ap(records):
    """sum over the distinct thresholds t, descending, of (R_t - R_prev) * P_t, each from a full count at t"""
    pos = sum(1 for _, tp in records if tp)
    if pos == 0:
        return float("nan")
    ap, prev = 0.0, 0.0
    for t in sorted({c for c, _ in records}, reverse=True):
        tp = sum(1 for c, y in records if c >= t and y)
        n = sum(1 for c, _ in records if c >= t)
        ap += (tp / pos - prev) * (tp / n)
        prev = tp / pos
    return ap


def _brute_auroc(cases):
    pos, neg = [s for s, y in cases if y], [s for s, y in cases if not y]
    if not pos or not neg:
        return float("nan")
    return sum(1.0 if a > b else 0.5 if a == b else 0.0 for a in pos for b in neg) / (len(pos) * len(neg))


def _cases(seed):
    """a list of (conf_tp, missed, case_label or None) with ties within and across cases"""
    rng = np.random.default_rng(seed)
    grid = [0.1, 0.25, 0.25, 0.5, 0.7, 0.7, 0.9]
    out = []
    for _ in range(int(rng.integers(4, 14))):
        k = int(rng.integers(0, 5))
        conf_tp = [(float(rng.choice(grid)) if rng.random() < 0.7 else float(rng.random()), bool(rng.random() < 0.5))
                   for _ in range(k)]
        out.append((conf_tp, int(rng.integers(0, 3)), None))
    return out


def _fill(cases):
    from hdf_rt import DetectionEvaluator
    ev = DetectionEvaluator()
    for conf_tp, missed, label in cases:
        ev.add_case(_match(conf_tp, missed), label)
    return ev


@pytest.mark.parametrize("seed", range(12))
def test_evaluator_against_brute_force_and_sklearn(seed):
    cases = _cases(seed)
    ev = _fill(cases)
    records = [r for conf_tp, missed, _ in cases for r in list(conf_tp) + [(0.0, True)] * missed]
    case_recs = [(max([c for c, _ in conf_tp], default=0.0), any(tp for _, tp in conf_tp) or missed > 0) for conf_tp, missed, _ in cases]
    assert sorted(ev.lesions) == sorted(records) and ev.cases == case_recs
    for got, want in ((ev.ap(), _brute_ap(records)), (ev.auroc(), _brute_auroc(case_recs))):
        assert (math.isnan(got) and math.isnan(want)) or abs(got - want) <= 1e-12, (got, want)
    if not math.isnan(ev.ap()) and not math.isnan(ev.auroc()):
        assert abs(ev.score() - (ev.ap() + ev.auroc()) / 2) <= 1e-15
    # FROC: every distinct confidence of a predicted lesion, from full counts
    preds = [r for conf_tp, _, _ in cases for r in conf_tp]
    n_truth = sum(sum(1 for _, tp in conf_tp if tp) + missed for conf_tp, missed, _ in cases)
    froc = ev.froc()
    ts = sorted({c for c, _ in preds}, reverse=True)
    assert froc["thresholds"] == ts
    for t, s, f in zip(ts, froc["sensitivity"], froc["fp_per_case"]):
        assert f == sum(1 for c, y in preds if c >= t and not y) / len(cases)
        if n_truth:
            assert s == sum(1 for c, y in preds if c >= t and y) / n_truth
    try:
        from sklearn.metrics import average_precision_score, roc_auc_score
    except ImportError:
        return
    if any(y for _, y in records):
        assert abs(ev.ap() - average_precision_score([y for _, y in records], [c for c, _ in records])) <= 1e-12
    if len({y for _, y in case_recs}) == 2:
        assert abs(ev.auroc() - roc_auc_score([y for _, y in case_recs], [s for s, _ in case_recs])) <= 1e-12


def test_evaluator_edge_cases():
    from hdf_rt import DetectionEvaluator
    ev = DetectionEvaluator()
    assert math.isnan(ev.ap()) and math.isnan(ev.auroc()) and ev.froc() == dict(thresholds=[], sensitivity=[], fp_per_case=[])
    ev = _fill([([(0.5, True)], 0, None), ([(0.5, True), (0.9, True)], 1, None)])          # positives only
    assert math.isnan(ev.auroc()) and math.isnan(ev.score())
    assert ev.ap() == pytest.approx(1 / 4 * 1 + 2 / 4 * 1 + 1 / 4 * 1, abs=1e-15)           # 0.9; the two 0.5 together; the miss at 0
    ev = _fill([([(0.5, False)], 0, None), ([], 0, None)])                                # negatives only
    assert math.isnan(ev.ap()) and math.isnan(ev.auroc()) and ev.cases == [(0.5, False), (0.0, False)]
    ev = _fill([([(0.4, True)], 0, None), ([(0.4, False)], 0, None)])                     # all tied
    assert ev.auroc() == 0.5 and ev.ap() == 0.5
    ev = _fill([([(0.4, False)], 0, True), ([(0.6, False)], 0, False)])                   # the caller's case labels
    assert ev.auroc() == 0.0
    with pytest.raises(ValueError):
        ev.add_case(dict(pred_match=[(0, 0.0)], truth_match=[], confidence=None))


# ------------------------------------------------------------------------------------------------------ the matching
ROWS = [[0, 1, 30, 0], [0, 2, 12, 0], [0, 4, 9, 0], [1, 0, 10, 0], [1, 1, 20, 0], [1, 2, 4, 0], [2, 0, 3, 0], [2, 2, 12, 0],
        [3, 0, 25, 0], [4, 1, 20, 0], [4, 3, 5, 0], [5, 3, 5, 0], [6, 0, 7, 0], [6, 3, 1, 0]]
SIZES = dict(pred_size=[34, 15, 25, 25, 5, 8], truth_size=[70, 28, 11, 9])
# what match_components' host half gave for ROWS (6 predicted, 4 truth lesions) before it moved into lesions._match_rows
RECORDED = {
    ("iou", 0.1): dict(tp=3, fp=3, fn=1, truth_match=[(4, 0.26666666666666666), (2, 0.3870967741935484), (5, 0.45454545454545453), (0, 0.0)],
                       pred_match=[(0, 0.0), (2, 0.3870967741935484), (0, 0.0), (1, 0.26666666666666666), (3, 0.45454545454545453), (0, 0.0)]),
    ("dice", 0.3): dict(tp=3, fp=3, fn=1, truth_match=[(4, 0.42105263157894735), (2, 0.5581395348837209), (5, 0.625), (0, 0.0)],
                        pred_match=[(0, 0.0), (2, 0.5581395348837209), (0, 0.0), (1, 0.42105263157894735), (3, 0.625), (0, 0.0)]),
    ("any", 0.9): dict(tp=3, fp=3, fn=1, truth_match=[(4, 0.26666666666666666), (2, 0.3870967741935484), (5, 0.45454545454545453), (0, 0.0)],
                       pred_match=[(0, 0.0), (2, 0.3870967741935484), (0, 0.0), (1, 0.26666666666666666), (3, 0.45454545454545453), (0, 0.0)]),
    ("iou", 0.45): dict(tp=1, fp=5, fn=3, truth_match=[(0, 0.0), (0, 0.0), (5, 0.45454545454545453), (0, 0.0)],
                        pred_match=[(0, 0.0), (0, 0.0), (0, 0.0), (0, 0.0), (3, 0.45454545454545453), (0, 0.0)]),
}


def test_match_candidates_host_half_against_the_recorded_dicts():
    from hdf_rt import detection, lesions
    cands = [dict(index=i, confidence=c, status="kept") for i, c in ((1, 0.9), (2, 0.8), (0, 0.75), (3, 0.7), (4, 0.6), (5, 0.5), (6, 0.4))]
    for (mode, thr), want in RECORDED.items():
        want = dict(want, **SIZES)
        assert lesions._match_rows(ROWS, 6, 4, thr, mode) == dict(want, confidence=None)
        assert detection._match_candidate_rows(ROWS, 4, cands, thr, mode) == dict(want, confidence=[0.9, 0.8, 0.7, 0.6, 0.5, 0.4])
        assert detection._match_candidate_rows(ROWS, 4, None, thr, mode) == dict(want, confidence=None)
    # a kept candidate without a voxel in the table's rows still is a predicted lesion, unmatched
    more = cands + [dict(index=7, confidence=0.3, status="kept")]
    got = detection._match_candidate_rows(ROWS, 4, more, 0.1, "iou")
    assert got["fp"] == 4 and got["pred_match"][6] == (0, 0.0) and got["pred_size"][6] == 0 and got["confidence"][6] == 0.3
    with pytest.raises(ValueError):
        detection._match_candidate_rows(ROWS, 4, cands[:3], 0.1, "iou")


def test_the_detection_functions_are_exported_and_need_a_gpu():
    import torch

    import hdf_rt
    for name in ("extract_lesion_candidates", "match_candidates", "DetectionEvaluator"):
        assert name in dir(hdf_rt) and callable(getattr(hdf_rt, name))
    assert {"hdf_detect_workspace_bytes", "hdf_detect_candidates"} <= set(hdf_rt.EXPORTS)
    # the workspace: 256 bytes of state, w, the mask, the ids and the labelling's own, each part on a 256-byte boundary
    up = lambda b: (b + 255) // 256 * 256
    for dims in ((1, 1, 1), (5, 17, 33), dr.BIG):
        V = int(np.prod(dims))
        assert hdf_rt.lib().hdf_detect_workspace_bytes(*dims) == 256 + 2 * up(4 * V) + up(V) + hdf_rt.lib().hdf_cc_workspace_bytes(*dims)
    assert hdf_rt.lib().hdf_detect_workspace_bytes(0, 4, 4) == -1 and hdf_rt.lib().hdf_last_error().startswith(b"detect:")
    if not torch.cuda.is_available():
        with pytest.raises(hdf_rt.HdfError):
            hdf_rt.extract_lesion_candidates(np.zeros((2, 3, 4), np.float32))
        with pytest.raises(hdf_rt.HdfError):
            hdf_rt.match_candidates(torch.zeros((2, 3, 4), dtype=torch.int32), np.zeros((2, 3, 4), np.uint8))
