"""Lesion candidates from a probability map on the device (csrc/detect.hip, hdf_rt.detection) against the numpy restatement
tests/detect_ref.py, itself held to a literal scipy loop by tests/test_detect_ref_cpu.py.

Every comparison is for equality in every bit -- detection_map, indexed, the table with the bits of m and of thr, the
result words: there is no floating arithmetic beyond one fp64 division and one comparison, so there is no tolerance.

Shapes (detect_ref.SHAPES): (1,1,1); (1,1,65), one voxel more than a wave; (1,40,70), the 2-D case; (5,17,33), (12,24,37)
and (9,65,31), odd rows over several workgroups; (3,5,257), rows one voxel longer than a workgroup.  The voxel passes of
detect.hip run at most HDF_DETECT_GRID_CAP = 2048 workgroups of 256: detect_ref.BIG = (9,241,243) has 527 067 voxels, more
than 2048 * 256 = 524 288, so their grid-stride loops make a second trip, and its only peak is the last voxel.
Inputs (detect_ref.KINDS): Gaussian blobs with 0.5 % noise; all zeros; one voxel; a plateau whose maximum lies at several
voxels of two components, with one voxel exactly on the threshold; two boxes that share a corner; a blob across a bar,
whose removal splits the next mask; NaN, negative, -0 and +-inf voxels; a peak below `stop`.
Parameters (detect_ref.PARAMS): num_lesions 1 and 5, factor 2.5 and 1.0000001, connectivity 6 / 18 / 26, remove_adjacent
on and off, min_voxels 0 and 10.

Every call is made twice into the same workspace, which is filled with 0x5A once and never cleared; both results must
agree in every bit.  Outputs are pre-filled with a marker and carry a guard tail.  Nothing here measures time."""
import numpy as np
import pytest
import torch
from scipy import ndimage as ndi

pytestmark = pytest.mark.gpu

import detect_ref as dr  # noqa: E402
from hdf_rt import detection  # noqa: E402
from hdf_rt._lib import lib, ptr  # noqa: E402
from hip_util import DEV, st  # noqa: E402

GUARD = 64
FIN = {0: "rounds", 1: "count", 2: "stop"}
_ws = {}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _workspace(dims):
    if dims not in _ws:
        n = lib().hdf_detect_workspace_bytes(*dims)
        assert n > 0
        _ws[dims] = torch.full((n,), 0x5A, dtype=torch.uint8, device=DEV)
    return _ws[dims]


class Buffers:
    """the outputs of a call, pre-filled with a marker, with a guard tail each"""

    def __init__(self, dims, table_rows, marker):
        self.dims, self.V, self.rows, self.marker = dims, int(np.prod(dims)), table_rows, marker
        self.det = torch.full((self.V + GUARD,), float(marker), dtype=torch.float32, device=DEV)
        self.idx = torch.full((self.V + GUARD,), marker, dtype=torch.int32, device=DEV)
        self.table = torch.full((table_rows * 6 + GUARD,), marker, dtype=torch.int64, device=DEV)
        self.res = torch.full((4 + GUARD,), marker, dtype=torch.int64, device=DEV)

    def call(self, p, params, first_round, rounds, stop=0.01, ws=None):
        n, f, c, ra, mv = params
        ws = _workspace(self.dims) if ws is None else ws
        rc = lib().hdf_detect_candidates(ptr(p), *self.dims, n, f, stop, c, ra, mv, first_round, rounds, ptr(self.det),
                                         ptr(self.idx), ptr(self.table), self.rows, ptr(self.res), ptr(ws), ws.numel(), st())
        assert rc == 0, lib().hdf_last_error()
        return self.res[:4].cpu().tolist()

    def outputs(self, words):
        """(det, idx, table rows, finished) on the host, after a look at the guards"""
        det, idx, table, res = self.det.cpu().numpy(), self.idx.cpu().numpy(), self.table.cpu().numpy(), self.res.cpu().numpy()
        assert (det[self.V:] == self.marker).all() and (idx[self.V:] == self.marker).all(), "write past the end of a map"
        assert (table[self.rows * 6:] == self.marker).all() and (res[4:] == self.marker).all(), "write past the table or result"
        rows = table[:self.rows * 6].reshape(-1, 6)
        assert not rows[words[0]:].any(), "a row behind the rounds run is not zero"
        return det[:self.V].reshape(self.dims), idx[:self.V].reshape(self.dims), rows[:words[0]], FIN[words[2]]


def _run(p_dev, dims, params, sync_every=8, max_rounds=dr.MAX_ROUNDS, marker=-5):
    """the chunked loop of extract_lesion_candidates on guarded buffers: (outputs, words)"""
    buf = Buffers(dims, max_rounds, marker)
    done = 0
    while True:
        words = buf.call(p_dev, params, done, min(sync_every, max_rounds - done))
        assert words[2] in (0, 1, 2) and words[3] == 0
        done = words[0]
        if words[2] != 0 or done >= max_rounds:
            return buf.outputs(words), words


@pytest.mark.parametrize("shape", dr.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_bit_against_the_restatement(shape):
    for kind in dr.KINDS:
        p = _dev(dr.volume(kind, shape))
        for params in dr.PARAMS:
            want = dr.reference(kind, shape, params)
            got, words = _run(p, shape, params, marker=-5)
            assert dr.same(got, want) == [], (kind, params, words, got[2], want[2])
            assert words[0] == len(want[2]) and words[1] == int(want[1].max())
            again, words2 = _run(p, shape, params, marker=-9)
            assert dr.same(again, got) == [] and words2 == words, ("two calls differ", kind, params)
        assert np.array_equal(p.cpu().numpy().view(np.uint32), dr.volume(kind, shape).view(np.uint32)), "the input changed"


def test_a_volume_larger_than_one_trip_of_the_grid():
    """HDF_DETECT_GRID_CAP = 2048 workgroups of 256 threads cover 524 288 voxels a trip; (9,241,243) has 527 067, and its
    only peak is the last one"""
    assert int(np.prod(dr.BIG)) > dr.GRID_CAP * 256
    p = _dev(dr.big_volume())
    for params in (dr.PARAMS[0], dr.PARAMS[5]):
        want = dr.reference("big", dr.BIG, params)
        got, words = _run(p, dr.BIG, params)
        assert dr.same(got, want) == [], (params, words, got[2], want[2])
        assert got[2][0][3] == int(np.prod(dr.BIG)) - 1
        again, _ = _run(p, dr.BIG, params, marker=-9)
        assert dr.same(again, got) == []


@pytest.mark.parametrize("shape", [(5, 17, 33), (1, 40, 70)], ids=lambda s: "x".join(map(str, s)))
def test_chunking_changes_nothing(shape):
    for kind in ("blobs", "specials", "split", "zeros"):
        p = _dev(dr.volume(kind, shape))
        for params in (dr.PARAMS[0], dr.PARAMS[4], dr.PARAMS[8], dr.PARAMS[10]):
            want = dr.reference(kind, shape, params)
            for sync_every in (1, 3, 8, dr.MAX_ROUNDS):
                got, words = _run(p, shape, params, sync_every=sync_every)
                assert dr.same(got, want) == [], (kind, params, sync_every, words)


def test_rounds_after_the_finish_change_nothing():
    shape = (12, 24, 37)
    for kind, params in (("blobs", dr.PARAMS[0]), ("blobs", dr.PARAMS[4]), ("zeros", dr.PARAMS[0])):
        p = _dev(dr.volume(kind, shape))
        want = dr.reference(kind, shape, params)
        assert want[3] in ("count", "stop")
        buf = Buffers(shape, dr.MAX_ROUNDS, -5)
        words = buf.call(p, params, 0, dr.MAX_ROUNDS)            # the finish lies inside this call: rounds run behind it
        assert dr.same(buf.outputs(words), want) == [] and words[0] == len(want[2]) < dr.MAX_ROUNDS
        snap = [t.clone() for t in (buf.det, buf.idx, buf.table)]
        for _ in range(2):                                       # and in later calls
            more = buf.call(p, params, words[0], 3)
            assert more == words
            assert all(torch.equal(a, b) for a, b in zip(snap, (buf.det, buf.idx, buf.table)))


def test_first_round_must_be_the_rounds_run_so_far():
    shape = (5, 17, 33)
    params = dr.PARAMS[4]
    p = _dev(dr.volume("blobs", shape))
    want = dr.reference("blobs", shape, params)
    assert len(want[2]) > 4
    buf = Buffers(shape, dr.MAX_ROUNDS, -5)
    words = buf.call(p, params, 0, 2)
    assert words[0] == 2 and words[2] == 0
    snap = [t.clone() for t in (buf.det, buf.idx, buf.table)]
    for wrong in (1, 3, 40):
        bad = buf.call(p, params, wrong, 2)
        assert bad == [2, words[1], 3, 0], (wrong, bad)
        assert all(torch.equal(a, b) for a, b in zip(snap, (buf.det, buf.idx, buf.table)))
    words = buf.call(p, params, 2, dr.MAX_ROUNDS - 2)            # the right one goes on where the state stands
    assert dr.same(buf.outputs(words), want) == []
    # a workspace that holds no state
    fresh = torch.full_like(_workspace(shape), 0x5A)
    buf = Buffers(shape, 4, -5)
    assert buf.call(p, params, 1, 1, ws=fresh)[2] == 3
    assert (buf.det == -5).all() and (buf.idx == -5).all() and (buf.table == -5).all()


def test_max_rounds_reports_rounds():
    from hdf_rt import extract_lesion_candidates
    shape, bound = (5, 17, 33), 7
    p = dr.volume("blobs", shape)
    want_all = dr.extract_ref(p, 5, 1.0000001, 0.01, 6, True, 0, 256)
    assert len(want_all[2]) > bound                              # the restatement needs more rounds than the bound
    want = dr.extract_ref(p, 5, 1.0000001, 0.01, 6, True, 0, bound)
    assert want[3] == "rounds" and np.array_equal(want[2], want_all[2][:bound])
    for sync_every in (8, 3):
        got = extract_lesion_candidates(_dev(p), 5, 1.0000001, 0.01, 6, True, 0, max_rounds=bound, sync_every=sync_every)
        assert got["finished"] == "rounds" and got["rounds"] == bound
        assert got["candidates"] == detection.candidates_from_rows(want[2].tolist())
        assert np.array_equal(got["indexed"].cpu().numpy(), want[1])
        assert np.array_equal(got["detection_map"].cpu().numpy().view(np.uint32), want[0].view(np.uint32))


def test_a_table_shorter_than_the_rounds():
    shape = (12, 24, 37)
    params = dr.PARAMS[4]
    p = _dev(dr.volume("blobs", shape))
    want = dr.reference("blobs", shape, params)
    rounds = len(want[2])
    assert rounds > 4
    for table_rows in (3, 1, 0):
        buf = Buffers(shape, table_rows, -5)
        words = buf.call(p, params, 0, 4)
        words = buf.call(p, params, 4, dr.MAX_ROUNDS - 4)
        assert words == [rounds, int(want[1].max()), 1 if want[3] == "count" else 2, rounds - table_rows]
        det, idx, table, res = (t.cpu().numpy() for t in (buf.det, buf.idx, buf.table, buf.res))
        assert np.array_equal(table[:table_rows * 6].reshape(-1, 6), want[2][:table_rows]) and (table[table_rows * 6:] == -5).all()
        assert np.array_equal(idx[:buf.V].reshape(shape), want[1]) and (idx[buf.V:] == -5).all()
        assert np.array_equal(det[:buf.V].view(np.uint32).reshape(shape), want[0].view(np.uint32))
    # no table at all
    buf = Buffers(shape, 0, -5)
    rc = lib().hdf_detect_candidates(ptr(p), *shape, *params[:1], params[1], 0.01, *params[2:], 0, dr.MAX_ROUNDS, ptr(buf.det),
                                     ptr(buf.idx), None, 0, ptr(buf.res), ptr(_workspace(shape)), _workspace(shape).numel(), st())
    assert rc == 0 and buf.res[:4].cpu().tolist() == [rounds, int(want[1].max()), 1 if want[3] == "count" else 2, rounds]


def test_the_python_entry(monkeypatch):
    import hdf_rt
    from hdf_rt import extract_lesion_candidates
    shape = (9, 65, 31)
    p = dr.volume("blobs", shape)
    want = dr.extract_ref(p, 5, 2.5, 0.01, 6, True, 0, 256)
    copies = []
    real = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda t, *a, **k: (copies.append(t.numel()), real(t, *a, **k))[1])
    got = extract_lesion_candidates(_dev(p))
    monkeypatch.undo()
    assert got["detection_map"].is_cuda and got["indexed"].is_cuda and got["indexed"].dtype == torch.int32
    assert tuple(got["indexed"].shape) == shape and got["finished"] == want[3] and got["rounds"] == len(want[2])
    assert copies == [4] * (len(want[2]) // 8 + 1) + [6 * len(want[2])], copies       # result words a chunk, one table
    assert got["candidates"] == detection.candidates_from_rows(want[2].tolist())
    assert [c["status"] for c in got["candidates"]] == [detection.STATUS[s] for s in want[2][:, 4]]
    assert np.array_equal(got["indexed"].cpu().numpy(), want[1])
    assert np.array_equal(got["detection_map"].cpu().numpy().view(np.uint32), want[0].view(np.uint32))
    # a numpy array, [H, W], other parameters
    p2 = dr.volume("specials", (1, 40, 70))[0]
    want = dr.extract_ref(p2, 3, 2.5, 0.05, 26, False, 4, 256)
    got = hdf_rt.extract_lesion_candidates(p2, 3, 2.5, 0.05, 26, False, 4, sync_every=5)
    assert tuple(got["indexed"].shape) == (40, 70) and got["finished"] == want[3]
    assert got["candidates"] == detection.candidates_from_rows(want[2].tolist())
    assert np.array_equal(got["indexed"].cpu().numpy(), want[1][0])
    assert sum(1 for key in detection._workspaces if key[-3:] == shape) == 1
    with pytest.raises(ValueError):
        extract_lesion_candidates(_dev(p).double())
    with pytest.raises(hdf_rt.HdfError, match="detect:"):
        extract_lesion_candidates(_dev(p), num_lesions=0)


def _truth_for(shape, seed):
    """a uint8 truth map: some of the blobs of the input grown or moved, and one of its own"""
    p = dr.volume("blobs", shape)
    rng = np.random.default_rng(seed)
    truth = ndi.binary_dilation(p > 0.35, iterations=1)
    truth = np.roll(truth, int(rng.integers(-1, 2)), axis=2)
    lab, n = ndi.label(truth)
    if n > 1:
        truth[lab == int(rng.integers(1, n + 1))] = False            # one the model finds and the truth does not hold
    truth[dr._box(shape, (0, 0, 0), (1, 2, 2))] = True
    return truth.astype(np.uint8)


@pytest.mark.parametrize("shape", [(12, 24, 37), (1, 40, 70)], ids=lambda s: "x".join(map(str, s)))
def test_match_candidates_against_the_restatement(shape):
    from hdf_rt import DetectionEvaluator, extract_lesion_candidates, match_candidates
    p = dr.volume("blobs", shape)
    truth = _truth_for(shape, 3)
    ids_t, n_truth = ndi.label(truth, ndi.generate_binary_structure(3, 3))
    assert n_truth >= 2
    for ra in (True, False):
        det, idx, table, _ = dr.extract_ref(p, 5, 2.5, 0.01, 6, ra, 0, 256)
        got_c = extract_lesion_candidates(_dev(p), remove_adjacent=ra)
        n_pred = int(idx.max())
        conf = [float(np.uint32(r[1]).view(np.float32)) for r in table if r[0] > 0]
        for mode, thr in (("iou", 0.1), ("dice", 0.3), ("any", 0.1)):
            want = dr.match_ids_ref(idx, n_pred, ids_t, n_truth, thr, mode)
            got = match_candidates(got_c["indexed"], _dev(truth), got_c["candidates"], min_overlap=thr, overlap=mode)
            assert list(got) == ["tp", "fp", "fn", "truth_match", "pred_match", "pred_size", "truth_size", "confidence"]
            assert {k: got[k] for k in want} == want, (mode, got, want)
            assert got["confidence"] == conf
            bare = match_candidates(got_c["indexed"], truth, min_overlap=thr, overlap=mode)        # a host truth map, no candidates
            assert bare["confidence"] is None and {k: bare[k] for k in want} == want
        ev = DetectionEvaluator()
        ev.add_case(got)
        assert len(ev.lesions) == n_pred + got["fn"] and ev.cases == [(max(conf), True)]


def test_two_candidates_that_touch_stay_two():
    from hdf_rt import extract_lesion_candidates, match_candidates
    shape = (5, 17, 33)
    p = dr.volume("corner", shape)
    got_c = extract_lesion_candidates(_dev(p), remove_adjacent=False)
    assert [c["index"] for c in got_c["candidates"]] == [1, 2]
    truth = (p > 0).astype(np.uint8)                              # one truth lesion under 26: both boxes
    got = match_candidates(got_c["indexed"], truth, got_c["candidates"])
    assert got["pred_size"] == [8, 8] and got["truth_size"] == [16] and (got["tp"], got["fp"], got["fn"]) == (1, 1, 0)
    assert got["pred_match"] == [(1, 0.5), (0, 0.0)] and got["confidence"] == [float(np.float32(0.9)), float(np.float32(0.8))]


def _blob_pair(shape, seed):
    """(pred, truth, score): seeded ellipsoids, the prediction keeping most of them displaced or resized, missing some and
    adding some of its own; a non-negative fp32 score"""
    rng = np.random.default_rng(2000 + seed)
    grid = np.indices(shape).astype(np.float64)
    truth, pred = np.zeros(shape, np.uint8), np.zeros(shape, np.uint8)

    def ball(c, r):
        return sum(((grid[k] - c[k]) / r[k]) ** 2 for k in range(len(shape))) <= 1.0

    for _ in range(int(rng.integers(4, 10))):
        c = [rng.uniform(0, s) for s in shape]
        r = [rng.uniform(1.0, 4.5) for _ in shape]
        truth[ball(c, r)] = 1
        if rng.random() < 0.2:
            continue
        scale = rng.uniform(0.5, 1.4)
        pred[ball([a + rng.uniform(-2.0, 2.0) for a in c], [scale * v for v in r])] = 1
    for _ in range(int(rng.integers(0, 4))):
        pred[ball([rng.uniform(0, s) for s in shape], [rng.uniform(0.8, 2.5) for _ in shape])] = 1
    return pred, truth, rng.random(shape, dtype=np.float32)


@pytest.mark.parametrize("kind", ["blobs_3d", "blobs_2d", "empty_prediction"])
def test_match_components_is_unchanged(kind):
    """match_components' host half moved into a helper that match_candidates shares: every field is what the matching from
    per-lesion boolean masks gives, the overlaps to the last bit, in the same key order"""
    from hdf_rt import match_components
    shape = (60, 72) if kind == "blobs_2d" else (14, 36, 44)
    pred, truth, score = _blob_pair(shape, 4)
    if kind == "empty_prediction":
        pred = np.zeros_like(pred)
    vol = (lambda a: a[None]) if len(shape) == 2 else (lambda a: a)
    structure = ndi.generate_binary_structure(3, 3)
    ids_p, n_pred = ndi.label(vol(pred), structure)
    ids_t, n_truth = ndi.label(vol(truth), structure)
    assert n_truth >= 3 and (n_pred >= 3 or kind == "empty_prediction")
    conf = [float(vol(score)[ids_p == i].max()) for i in range(1, n_pred + 1)]
    for mode, thr in (("iou", 0.1), ("dice", 0.3), ("any", 0.1)):
        want = dr.match_ids_ref(ids_p, n_pred, ids_t, n_truth, thr, mode)
        got = match_components(_dev(pred), _dev(truth), score=_dev(score), min_overlap=thr, overlap=mode)
        assert list(got) == ["tp", "fp", "fn", "truth_match", "pred_match", "pred_size", "truth_size", "confidence"]
        assert {k: got[k] for k in want} == want, (mode, got, want)
        assert got["confidence"] == conf
    assert match_components(_dev(pred), _dev(truth))["confidence"] is None


def test_refusals():
    """every one returns HDF_ERR_ARG = 1 with a "detect:" message, before anything is launched: the outputs keep their marker"""
    shape = (3, 5, 7)
    V = 105
    p = _dev(dr.volume("blobs", shape))
    buf = Buffers(shape, 8, -5)
    ws = _workspace(shape)
    need = lib().hdf_detect_workspace_bytes(*shape)
    assert need == ws.numel() and need >= 256 + 9 * V + lib().hdf_cc_workspace_bytes(*shape)
    good = dict(prob=ptr(p), D=3, H=5, W=7, num_lesions=5, factor=2.5, stop=0.01, connectivity=6, remove_adjacent=1, min_voxels=0,
                first_round=0, rounds=2, det=ptr(buf.det), idx=ptr(buf.idx), table=ptr(buf.table), table_rows=8, res=ptr(buf.res),
                ws=ptr(ws), ws_bytes=ws.numel())

    def call(**kw):
        a = dict(good, **kw)
        rc = lib().hdf_detect_candidates(a["prob"], a["D"], a["H"], a["W"], a["num_lesions"], a["factor"], a["stop"], a["connectivity"],
                                         a["remove_adjacent"], a["min_voxels"], a["first_round"], a["rounds"], a["det"], a["idx"],
                                         a["table"], a["table_rows"], a["res"], a["ws"], a["ws_bytes"], st())
        return rc, lib().hdf_last_error().decode()

    inf, nan = float("inf"), float("nan")
    bad = [dict(D=0), dict(H=1025), dict(W=-1), dict(num_lesions=0), dict(factor=1.0), dict(factor=0.5), dict(factor=inf),
           dict(factor=nan), dict(stop=0.0), dict(stop=-1.0), dict(stop=inf), dict(stop=nan), dict(connectivity=8),
           dict(connectivity=0), dict(remove_adjacent=2), dict(min_voxels=-1), dict(rounds=0), dict(first_round=-1),
           dict(table_rows=-1), dict(prob=None), dict(det=None), dict(idx=None), dict(table=None), dict(res=None), dict(ws=None),
           dict(ws_bytes=need - 1), dict(ws=ptr(ws) + 4, ws_bytes=need + 8)]
    # any two of prob, detection_map, indexed, table, result and the workspace that share a byte
    big = torch.zeros(need + 4 * V + 64, dtype=torch.uint8, device=DEV)
    at = big.data_ptr()
    bad += [dict(det=ptr(p)), dict(idx=ptr(p)), dict(table=ptr(p)), dict(res=ptr(p) + 4 * V - 4), dict(prob=at + need - 8, ws=at),
            dict(idx=ptr(buf.det)), dict(table=ptr(buf.det) + 8), dict(res=ptr(buf.det)), dict(det=at + 8, ws=at),
            dict(table=ptr(buf.idx)), dict(res=ptr(buf.idx) + 16), dict(idx=at + need - 4, ws=at),
            dict(res=ptr(buf.table) + 8 * 47), dict(table=at + 256, ws=at), dict(res=at + need - 8, ws=at)]
    for kw in bad:
        rc, msg = call(**kw)
        assert rc == 1 and msg.startswith("detect:"), (kw, rc, msg)
    for dims in ((0, 5, 7), (3, 1025, 7)):
        assert lib().hdf_detect_workspace_bytes(*dims) == -1 and lib().hdf_last_error().decode().startswith("detect:")
    torch.cuda.synchronize()
    assert (buf.det == -5).all() and (buf.idx == -5).all() and (buf.table == -5).all() and (buf.res == -5).all()
    rc, msg = call()
    assert rc == 0, msg
