"""Per-lesion surface distances on crops (csrc/lesion_surface.hip, hdf_lesion_surface) and the lesion-wise HD95 of
hdf_rt.lesion_wise_scores(hd95=True) against the numpy / scipy restatement on FULL-VOLUME masks (tests/lesion_hd_ref.py,
itself held by tests/test_lesion_hd_ref_cpu.py) -- so equality also proves the crop.

Inputs (lesion_hd_ref.cases): lesion_ref.blob_pair with seeds 0..3 on (1,1,1) (both masks fill the volume), (1,9,33), (5,6,7),
(3,17,33), (8,8,70) (a crop row crosses a wave), (17,16,65) and (24,40,48) (crops of several workgroups), and the hand-made
cases: a lesion in a corner (three clamped sides), a predicted bar over two truth lesions (one id in two P_j, overlapping
crops), a miss and a lone false positive, no dilation, a min_size that drops a lesion, truth filling the volume, only false
positives, only misses, nothing, and a lattice of 100 one-voxel lesions (more than the 64 lesions of one carve launch, crops
of odd width whose predicted mask starts at an odd byte).

The entry: every one of the 12 x L result words equals the restatement's, both crops are read back from the workspace
(include/hdf.h states their layout) and equal the full-volume masks cut to the crop, and every call is made twice into the
same uncleared workspace (filled with 0x5A once) with identical results and crops.  The wrapper: the whole dict equals
lesion_hd_ref's -- ints, lists and None exactly, floats in every bit (lesion_hd_ref.mismatches): they are formed from equal
integers by the same fp64 expressions.  Nothing here measures time: the largest volume has 46 080 voxels."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import lesion_hd_ref as lh  # noqa: E402
import lesion_ref as lr  # noqa: E402
from hdf_rt._lib import check, lib, ptr  # noqa: E402
from hip_util import DEV, st  # noqa: E402

GUARD = 64
SPACINGS = [None, lh.SPACING]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _entry(name, spacing):
    """(result rows [L][12] as lists, the workspace bytes as numpy) of two calls that must agree in every byte"""
    _n, pred, _truth, _label, _kw = lh.case(name)
    shape = pred.shape
    e = lh.case_entry(name)
    L = len(e["lesions"])
    rows7 = (ctypes.c_int32 * max(7 * L, 1))(*[int(v) for v in e["lesions"].ravel()])
    sp = None if spacing is None else (ctypes.c_double * 3)(*spacing)
    need = lib().hdf_lesion_surface_workspace_bytes(rows7, L, *shape, 0 if sp is None else 1)
    assert need >= 0
    ids_p, ids_t, mask = _dev(e["ids_pred"]), _dev(e["ids_truth"]), _dev(e["mask"])
    n_pairs = e["n_pairs"]
    pairs = _dev(e["pairs"][:max(n_pairs, 1)])
    ws = torch.full((need + GUARD,), 0x5A, dtype=torch.uint8, device=DEV)
    got = []
    for marker in (-5, -9):
        res = torch.full((L * 12 + GUARD,), marker, dtype=torch.int64, device=DEV)
        check(lib().hdf_lesion_surface(ptr(ids_p), ptr(ids_t), ptr(mask), *shape, ptr(pairs), n_pairs, rows7, L, sp, ptr(ws), need,
                                       ptr(res), st()), "hdf_lesion_surface")
        r, w = res.cpu().numpy(), ws.cpu().numpy()
        assert (r[L * 12:] == marker).all() and (w[need:] == 0x5A).all(), "write past the end of an output"
        got.append((r[:L * 12].reshape(L, 12), w[:need]))
    assert np.array_equal(got[0][0], got[1][0]), "two calls differ in a result word"
    layout, total = lh.crop_layout(e["lesions"], shape)
    assert np.array_equal(got[0][1][:total], got[1][1][:total]), "two calls differ in a crop byte"
    return got[0][0].tolist(), got[0][1]


@pytest.mark.parametrize("spacing", SPACINGS, ids=["voxels", "mm"])
@pytest.mark.parametrize("name", lh.CASE_NAMES)
def test_entry_every_word_and_both_crops(name, spacing):
    rows, ws = _entry(name, spacing)
    want = lh.case_entry_words(name, spacing)
    assert rows == want, [(i, g, w) for i, (g, w) in enumerate(zip(rows, want)) if g != w][:3]
    e = lh.case_entry(name)
    layout, _total = lh.crop_layout(e["lesions"], lh.case(name)[1].shape)
    for (off, box), (T, P) in zip(layout, e["masks"]):
        n = T[box].size
        assert np.array_equal(ws[off: off + n], T[box].astype(np.uint8).ravel()), (name, off, "truth crop")
        assert np.array_equal(ws[off + n: off + 2 * n], P[box].astype(np.uint8).ravel()), (name, off, "predicted crop")


def test_entry_takes_a_larger_box_and_an_unlisted_pair():
    """any box that contains the lesion gives the same words (the whole volume too), and a predicted id whose pair row is
    missing from the table is outside P_j"""
    name = "bar"
    e = lh.case_entry(name)
    shape = lh.case(name)[1].shape
    whole = e["lesions"].copy()
    whole[:, 1:] = [0, shape[0] - 1, 0, shape[1] - 1, 0, shape[2] - 1]
    ids_p, ids_t, mask = _dev(e["ids_pred"]), _dev(e["ids_truth"]), _dev(e["mask"])

    def run(lesions, pairs):
        L = len(lesions)
        rows7 = (ctypes.c_int32 * (7 * L))(*[int(v) for v in lesions.ravel()])
        need = lib().hdf_lesion_surface_workspace_bytes(rows7, L, *shape, 0)
        ws = torch.empty(need, dtype=torch.uint8, device=DEV)
        res = torch.empty((L, 12), dtype=torch.int64, device=DEV)
        dp = _dev(pairs) if len(pairs) else None
        check(lib().hdf_lesion_surface(ptr(ids_p), ptr(ids_t), ptr(mask), *shape, ptr(dp), len(pairs), rows7, L, None, ptr(ws),
                                       need, ptr(res), st()), "hdf_lesion_surface")
        return res.cpu().tolist()

    listed = e["pairs"][:e["n_pairs"]]
    assert run(whole, listed) == lh.case_entry_words(name)
    # without the rows (1, j): P_j is empty -- words 1, 2 and 4 are zero, the pair of masks is invalid
    cut = listed[listed[:, 0] != 1]
    for row, full in zip(run(e["lesions"], cut), lh.case_entry_words(name)):
        assert row[0] == full[0] and row[3] == full[3] and [row[k] for k in (1, 2, 4, 11)] == [0, 0, 0, 0]
    assert run(e["lesions"], cut[:0])[0][1] == 0          # no rows at all, a null table


@pytest.mark.parametrize("spacing", SPACINGS, ids=["voxels", "mm"])
@pytest.mark.parametrize("name", lh.CASE_NAMES)
def test_lesion_wise_scores_hd95_equals_the_restatement(name, spacing):
    from hdf_rt import lesion_wise_scores
    _n, pred, truth, label, kw = lh.case(name)
    dp, dt = _dev(pred), _dev(truth)
    want = lh.case_ref(name, spacing)
    got = lesion_wise_scores(dp, dt, label, hd95=True, spacing=spacing, **kw)
    assert lh.mismatches(got, want) == [], (lh.mismatches(got, want)[:4], got["lesion_hd95"], want["lesion_hd95"])
    assert lh.mismatches(lesion_wise_scores(dp, dt, label, hd95=True, spacing=spacing, **kw), got) == [], "two calls differ"
    if spacing is None:
        # hd95=False is today's dict: the restatement of the Dice half, key for key, and nothing of the new half
        plain = lesion_wise_scores(dp, dt, label, **kw)
        assert lh.mismatches(plain, lr.lesion_wise_ref(pred, truth, label, **kw)) == []
        assert lh.mismatches(lesion_wise_scores(dp, dt, label, hd95=False, **kw), plain) == []


def test_penalty_spacing_without_hd95_and_capacity():
    from hdf_rt import HdfError, lesion_wise_scores
    _n, pred, truth, label, kw = lh.case("miss_and_fp")
    want = lh.lesion_hd_ref(pred, truth, label, hd95_penalty=50.5, spacing=lh.SPACING, **kw)
    got = lesion_wise_scores(pred, truth, label, hd95=True, hd95_penalty=50.5, spacing=lh.SPACING, **kw)
    assert lh.mismatches(got, want) == [] and 50.5 in [l["hd95"] for l in got["lesions"]]
    with pytest.raises(ValueError, match="hd95=True"):
        lesion_wise_scores(pred, truth, label, spacing=lh.SPACING, **kw)
    with pytest.raises(HdfError, match="spacing"):
        lesion_wise_scores(pred, truth, label, hd95=True, spacing=(0.0, 1.0, 1.0), **kw)
    with pytest.raises(HdfError, match="capacity 2"):
        lesion_wise_scores(pred, truth, label, hd95=True, capacity=2, **kw)
    # a [H, W] pair is the depth-1 volume
    p2, t2 = pred[4], truth[4]
    assert lh.mismatches(lesion_wise_scores(p2, t2, label, hd95=True, **kw), lh.lesion_hd_ref(p2, t2, label, **kw)) == []


def test_hd95_path_waits_for_the_host_twice_only(monkeypatch):
    """no torch.cuda.synchronize, and exactly two device-to-host copies: the tables, then the result rows"""
    from hdf_rt import lesion_wise_scores
    _n, pred, truth, label, kw = lh.case("24x40x48-s2")
    dp, dt = _dev(pred), _dev(truth)
    copies = []
    real_cpu = torch.Tensor.cpu

    def counting_cpu(self, *a, **k):
        copies.append(tuple(self.shape))
        return real_cpu(self, *a, **k)

    def no_sync(*a, **k):
        raise AssertionError("torch.cuda.synchronize called")
    monkeypatch.setattr(torch.cuda, "synchronize", no_sync)
    monkeypatch.setattr(torch.Tensor, "cpu", counting_cpu)
    got = lesion_wise_scores(dp, dt, label, hd95=True, **kw)
    plain_from = len(copies)
    lesion_wise_scores(dp, dt, label, **kw)
    monkeypatch.undo()
    scored = [l for l in got["lesions"] if l["pred"]]
    assert plain_from == 2 and copies[1] == (len(scored), 12) and len(copies) == 3, copies
