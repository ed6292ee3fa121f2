"""The overlap table of two id maps on the device (csrc/cc_pairs.hip) and the lesion-wise protocols of hdf_rt.lesions
against the numpy / scipy restatement (tests/lesion_ref.py, itself held to a triple loop and to hand-worked cases by
tests/test_lesion_ref_cpu.py).

Shapes (lesion_ref.SHAPES): (1,1,1); (1,1,63), (1,1,64), (1,1,65), the wave edge; (1,3,70) and (2,5,37), where a wave spans
row starts with the same pair on both sides of the break; (1,40,40), the 2-D case; (3,17,33); (9,20,257), rows one voxel
longer than the 256 voxels a workgroup reads per trip, six workgroup spans of 8192; (24,40,48); (8,32,32), one span
exactly; (1,9,911) and (5,29,113), whose last workgroup holds seven voxels and one (the geometry is read from
csrc/cc_pairs.h: lesion_ref.geometry, checked against the shapes in tests/test_lesion_ref_cpu.py).
Maps (lesion_ref.MAPS): both empty, one empty, one pair filling the volume, labelings of random blobs by hdf_cc_label, the
synthetic maps a = 1 + v // 3, b = 1 + v // 5 (thousands of pairs in a workgroup's span against its 256 LDS slots), ids_a
is ids_b, negative ids sprinkled in -- each without a mask and under a random, an all-zero and an all-255 mask, and under
all four flag values.

Every comparison is exact (lesion_ref.mismatches): each int64 of pairs and each word of result.  Every call is made twice
into the same workspace, which is filled with 0x5A once and never cleared, and both results must agree in every word.
Outputs are pre-filled with a marker and carry a guard tail.  Nothing here measures time: the largest volume has 46 260
voxels."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import lesion_ref as lr  # noqa: E402
from hdf_rt import lesions  # noqa: E402
from hdf_rt._lib import check, lib, ptr  # noqa: E402
from hip_util import DEV, st  # noqa: E402

GUARD = 64
GEO = lr.geometry()
_ws = {}


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _workspace(cap):
    if cap not in _ws:
        n = lib().hdf_cc_pairs_workspace_bytes(cap)
        assert n > 0
        _ws[cap] = torch.full((n,), 0x5A, dtype=torch.uint8, device=DEV)
    return _ws[cap]


def _pairs(a, b, mask, flags, shape, cap):
    """(pairs, result) of two calls into the same uncleared workspace, which must agree in every word"""
    ws = _workspace(cap)
    got = []
    for marker in (-5, -9):
        pairs = torch.full((cap * 4 + GUARD,), marker, dtype=torch.int64, device=DEV)
        res = torch.full((5,), -7, dtype=torch.int64, device=DEV)
        check(lib().hdf_cc_pairs(ptr(a), ptr(b), ptr(mask), flags, *shape, cap, ptr(pairs), ptr(res), ptr(ws), ws.numel(), st()),
              "hdf_cc_pairs")
        p, r = pairs.cpu().numpy(), res.cpu().tolist()
        assert (p[cap * 4:] == marker).all() and r[4] == -7, "write past the end of an output"
        got.append((p[:cap * 4].reshape(cap, 4), r[:4]))
    assert np.array_equal(got[0][0], got[1][0]) and got[0][1] == got[1][1], "two calls differ"
    return got[0]


def _maps(shape, kind):
    """(device a, device b, host a, host b); 'blobs': the ids hdf_cc_label gives two blob maps"""
    if kind == "blobs":
        from hdf_rt import connected_components
        a = connected_components(_dev(lr.blobs(shape, 11 + sum(shape), 9)))[0]
        b = connected_components(_dev(lr.blobs(shape, 12 + sum(shape), 9)))[0]
        ha, hb = lr.id_maps(shape, kind)
        assert np.array_equal(a.cpu().numpy(), ha) and np.array_equal(b.cpu().numpy(), hb)
        return a, b, ha, hb
    ha, hb = lr.id_maps(shape, kind)
    a = _dev(ha)
    return a, (a if kind == "same" else _dev(hb)), ha, hb


@pytest.mark.parametrize("shape", lr.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pairs_every_word(shape):
    for kind in lr.MAPS:
        a, b, ha, hb = _maps(shape, kind)
        for mk in lr.MASKS:
            hm = lr.mask_of(shape, mk)
            m = _dev(hm)
            for flags in lr.FLAGS:
                want = lr.pairs_ref(ha, hb, hm, flags, 4096)
                got = _pairs(a, b, m, flags, shape, 4096)
                assert lr.mismatches(got, want) == [], (kind, mk, flags, got[1])
                if want[1][3] and flags == 3:              # more than 4096 pairs: once with room for them too
                    got = _pairs(a, b, m, flags, shape, 32768)
                    assert lr.mismatches(got, lr.pairs_ref(ha, hb, hm, flags, 32768)) == [], (kind, mk, flags, got[1])


@pytest.mark.parametrize("shape", lr.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_capacities_and_the_exact_overflow_flag(shape):
    """capacity 1, the exact P of the case (no overflow) and P - 1 (overflow: every row and result[0..2] zero, result[3] = 1)"""
    hm = lr.mask_of(shape, "random")
    m = _dev(hm)
    for kind in lr.MAPS:
        a, b, ha, hb = _maps(shape, kind)
        for flags in (0, 3):
            P = lr.pairs_ref(ha, hb, hm, flags, 1 << 16)[1][0]
            if kind == "synthetic" and P > 4096:
                continue                                   # (the sort across workgroups: the test below)
            for cap in sorted({1, max(P, 1), max(P - 1, 1)}):
                want = lr.pairs_ref(ha, hb, hm, flags, cap)
                got = _pairs(a, b, m, flags, shape, cap)
                assert lr.mismatches(got, want) == [], (kind, flags, cap, P, got[1])
                if P > cap:
                    assert got[1] == [0, 0, 0, 1] and not got[0].any()
                else:
                    assert got[1][0] == P and got[1][3] == 0


def test_more_pairs_than_one_workgroup_sorts():
    """the synthetic maps on (24,40,48) hold 21 504 distinct pairs: capacities whose tables are 8 and 16 chunks of the
    single-workgroup sort, at the exact P, one below it, and with room to spare"""
    shape = lr.SORT_SHAPE
    a, b, ha, hb = _maps(shape, "synthetic")
    hm = lr.mask_of(shape, "random")
    m = _dev(hm)
    P = lr.pairs_ref(ha, hb, hm, 3, 1 << 16)[1][0]
    assert P == 21504 > GEO["SORT_CHUNK"]
    for cap in (P, P - 1, 32768, 65536):
        assert lib().hdf_cc_pairs_workspace_bytes(cap) >= 256 + 24 * 4 * GEO["SORT_CHUNK"]
        for mask, hmask in ((m, hm), (None, None)):
            got = _pairs(a, b, mask, 3, shape, cap)
            assert lr.mismatches(got, lr.pairs_ref(ha, hb, hmask, 3, cap)) == [], (cap, got[1])
    # and a workgroup's span holds more distinct pairs than it has LDS slots
    assert len(np.unique((ha.ravel()[:GEO["SPAN"]].astype(np.int64) << 32) | hb.ravel()[:GEO["SPAN"]])) > GEO["LDS_SLOTS"]


def test_a_mask_that_aliases_an_id_map():
    """the mask is an input like the id maps: it may be the first V bytes of ids_a itself"""
    shape = (3, 17, 33)
    ha, hb = lr.id_maps(shape, "negative")
    a, b = _dev(ha), _dev(hb)
    V = ha.size
    m = a.view(torch.uint8).reshape(-1)[:V]
    assert m.data_ptr() == a.data_ptr()
    hm = ha.view(np.uint8).reshape(-1)[:V].reshape(shape)
    for flags in lr.FLAGS:
        assert lr.mismatches(_pairs(a, b, m, flags, shape, 4096), lr.pairs_ref(ha, hb, hm, flags, 4096)) == [], flags


# ------------------------------------------------------------------------------------------------ the Python surface
SEEDS = list(range(20))


def _blob_case(seed):
    shape = (14, 36, 44) if seed % 2 == 0 else (60, 72)          # 3-D and 2-D
    return lr.blob_pair(shape, seed)


def test_component_overlap_returns_device_tensors():
    from hdf_rt import component_overlap
    shape = (3, 17, 33)
    ha, hb = lr.id_maps(shape, "blobs")
    hm = lr.mask_of(shape, "random")
    pairs, res = component_overlap(_dev(ha), _dev(hb), _dev(hm), capacity=64, zero_a=True, zero_b=True)
    assert pairs.is_cuda and res.is_cuda and pairs.dtype == torch.int64 and tuple(pairs.shape) == (64, 4) and tuple(res.shape) == (4,)
    assert lr.mismatches((pairs.cpu().numpy(), res.cpu().tolist()), lr.pairs_ref(ha, hb, hm, 3, 64)) == []
    p2, r2 = component_overlap(_dev(ha[0]), _dev(hb[0]), hm[0] != 0, capacity=64)           # [H, W], a bool mask on the host
    assert lr.mismatches((p2.cpu().numpy(), r2.cpu().tolist()), lr.pairs_ref(ha[:1], hb[:1], hm[:1], 0, 64)) == []
    with pytest.raises(ValueError):
        component_overlap(_dev(ha), _dev(hb[:2]))
    assert sum(1 for key in lesions._workspaces if key[-1] == 64) == 1


@pytest.mark.parametrize("seed", SEEDS)
def test_match_components_against_the_restatement(seed):
    from hdf_rt import match_components
    pred, truth, score = _blob_case(seed)
    dp, dt, ds = _dev(pred), _dev(truth), _dev(score)
    for mode, thr in (("iou", 0.1), ("dice", 0.3), ("any", 0.1)):
        want = lr.match_ref(pred, truth, score=score, min_overlap=thr, overlap=mode)
        got = match_components(dp, dt, score=ds, min_overlap=thr, overlap=mode)
        for key in ("tp", "fp", "fn", "pred_size", "truth_size"):
            assert got[key] == want[key], (mode, key, got[key], want[key])
        for key in ("truth_match", "pred_match"):
            assert [i for i, _ in got[key]] == [i for i, _ in want[key]], (mode, key)
            assert all(abs(g - w) <= 1e-12 for (_, g), (_, w) in zip(got[key], want[key])), (mode, key)
        assert np.array_equal(np.asarray(got["confidence"], np.float32).view(np.int32),
                              np.asarray(want["confidence"], np.float32).view(np.int32)), mode
    assert match_components(dp, dt)["confidence"] is None
    assert want["tp"] + want["fn"] >= 1


@pytest.mark.parametrize("seed", SEEDS)
def test_lesion_wise_scores_against_the_restatement(seed):
    from hdf_rt import lesion_wise_scores
    pred, truth, _ = _blob_case(seed)
    dp, dt = _dev(pred), _dev(truth)
    for kw in (dict(), dict(dilate_iterations=1, dilate_connectivity=6, min_size=12), dict(dilate_iterations=0, connectivity=6)):
        want = lr.lesion_wise_ref(pred, truth, 1, **kw)
        got = lesion_wise_scores(dp, dt, 1, **kw)
        for key in ("dropped", "false_positives", "fp"):
            assert got[key] == want[key], (kw, key, got[key], want[key])
        assert len(got["lesions"]) == len(want["lesions"])
        for g, w in zip(got["lesions"], want["lesions"]):
            assert {k: g[k] for k in ("id", "gt", "tp", "pred", "pred_voxels")} == {k: w[k] for k in ("id", "gt", "tp", "pred", "pred_voxels")}, kw
            assert abs(g["dice"] - w["dice"]) <= 1e-12
        assert abs(got["lesion_dice"] - want["lesion_dice"]) <= 1e-12, (kw, got["lesion_dice"], want["lesion_dice"])
    # another class, and a class neither map holds
    p2, t2 = (pred * 2).astype(np.uint8), np.where(truth > 0, 2, 0).astype(np.uint8)
    assert lesion_wise_scores(p2, t2, 2)["lesion_dice"] == pytest.approx(lr.lesion_wise_ref(pred, truth, 1)["lesion_dice"], abs=1e-12)
    assert lesion_wise_scores(dp, dt, 7) == dict(lesions=[], dropped=[], false_positives=[], fp=0, lesion_dice=1.0)


def test_fill_holes_then_lesion_wise_scores_stays_on_the_device(monkeypatch):
    """fill_class_holes -> lesion_wise_scores on device tensors: nothing waits on the host before the one copy of the
    table -- torch.cuda.synchronize is never called, and the filled map never leaves the device"""
    from hdf_rt import fill_class_holes, lesion_wise_scores
    pred, truth, _ = lr.blob_pair((14, 36, 44), 2)
    from scipy import ndimage as ndi
    holed = pred.copy()
    inner = np.argwhere(ndi.binary_erosion(pred == 1, np.ones((3, 3, 3), bool)))
    assert len(inner)
    for z, y, x in inner[::7]:
        holed[z, y, x] = 0
    filled_ref = np.where(ndi.binary_fill_holes(holed == 1), 1, holed).astype(np.uint8)
    assert (filled_ref != holed).any()

    def no_sync(*a, **k):
        raise AssertionError("torch.cuda.synchronize called")
    monkeypatch.setattr(torch.cuda, "synchronize", no_sync)
    filled = fill_class_holes(_dev(holed), 1)
    assert filled.is_cuda
    got = lesion_wise_scores(filled, _dev(truth), 1)
    monkeypatch.undo()
    want = lr.lesion_wise_ref(filled_ref, truth, 1)
    assert np.array_equal(filled.cpu().numpy(), filled_ref)
    assert abs(got["lesion_dice"] - want["lesion_dice"]) <= 1e-12 and got["fp"] == want["fp"]
    assert [l["tp"] for l in got["lesions"]] == [l["tp"] for l in want["lesions"]]


def test_more_pairs_than_capacity_raises():
    from hdf_rt import HdfError, component_overlap, lesion_wise_scores, match_components
    pred, truth, _ = lr.blob_pair((14, 36, 44), 4)
    with pytest.raises(HdfError, match="capacity 2"):
        match_components(pred, truth, capacity=2)
    with pytest.raises(HdfError, match="capacity 2"):
        lesion_wise_scores(pred, truth, 1, capacity=2)
    with pytest.raises(HdfError):
        component_overlap(_dev(lr.id_maps((3, 17, 33), "blobs")[0]), _dev(lr.id_maps((3, 17, 33), "blobs")[1]), capacity=0)
    # the device entry itself reports the overflow in result[3] and raises nothing
    ha, hb = lr.id_maps((3, 17, 33), "synthetic")
    _, res = component_overlap(_dev(ha), _dev(hb), capacity=2)
    assert res.cpu().tolist() == [0, 0, 0, 1]
