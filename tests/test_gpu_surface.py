"""Surface-distance evaluation on the device (csrc/surface.hip, hdf_rt/surface.py) against the scipy restatement of the
definitions in include/hdf.h (tests/surface_ref.py, itself held to brute force by tests/test_surface_ref_cpu.py).

Shapes: the smallest that reach every tiling edge -- (1,1,1) and a depth-1 volume; (19,67,131), odd and across a wave
and a tile on every axis; (5,3,300), a line longer than 256 lanes; the cap of 1024 on each axis in turn (LDS tiles of 8
lines, sixteen ballot chunks a row) and (2,600,5) (tiles of 16); (40,48,56) with three labels through the multi_* wrappers.  Masks per shape
(surface_ref.MASKS): seeded blobs, blobs that run into the volume's faces, identical masks, one voxel in each of two
opposite corners (hd2 = sum (dim-1)^2: 1 046 534 at (1024,2,3), beside the no-seed sentinel in the same lines), two
distant slabs, empty T / P / both, a mask that fills the volume.

Every comparison is exact -- each flag byte, the five counts, each int32 of both distance maps, the whole histogram, the
twelve result integers -- except the wrappers' floats (1e-12 relative to the fp64 restatement; NaN exactly where the
definitions say).  Outputs are pre-filled with a marker and carry a guard tail, so an unwritten element or a write past
the end shows."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import surface_ref as sr  # noqa: E402
from hdf_rt._lib import check, lib, ptr  # noqa: E402
from hip_util import DEV, st  # noqa: E402

IDS = ["x".join(map(str, s)) for s in sr.SHAPES]
GUARD = 64


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _workspace(shape):
    n = lib().hdf_surface_workspace_bytes(*shape)
    assert n > 0
    return torch.full((n,), 0x5A, dtype=torch.uint8, device=DEV)


def _edt(flags, seed_bit, shape, ws):
    v = int(np.prod(shape))
    d2 = torch.full((v + GUARD,), -77, dtype=torch.int32, device=DEV)
    check(lib().hdf_op_edt_sq(ptr(flags), seed_bit, *shape, ptr(d2), ptr(ws), ws.numel(), st()), "hdf_op_edt_sq")
    out = d2.cpu().numpy()
    assert (out[v:] == -77).all(), "write past the end of d2"
    return out[:v].reshape(shape).astype(np.int64)


def _distances(t, p, k, shape, ws, extra=5):
    nb = sr.hist_bins(shape)
    res = torch.full((13,), -7, dtype=torch.int64, device=DEV)
    hist = torch.full((nb + extra + GUARD,), 0xABCD, dtype=torch.int32, device=DEV)
    check(lib().hdf_surface_distances(ptr(t), ptr(p), k, *shape, ptr(ws), ws.numel(), ptr(res), ptr(hist), nb + extra,
                                      st()), "hdf_surface_distances")
    res, hist = res.cpu().tolist(), hist.cpu().numpy().astype(np.int64)
    assert res[12] == -7 and (hist[nb + extra:] == 0xABCD).all(), "write past the end of an output"
    assert (hist[nb:nb + extra] == 0).all(), "entries past the last possible squared distance are 0"
    return res[:12], hist[:nb]


@pytest.mark.parametrize("shape", sr.SHAPES, ids=IDS)
def test_mask_flags_every_byte_and_all_five_counts(shape):
    v = int(np.prod(shape))
    for kind in sr.MASKS:
        t, p, k = sr.case(shape, kind)
        ref = sr.case_ref(shape, kind)
        flags = torch.full((v + GUARD,), 0xEE, dtype=torch.uint8, device=DEV)
        counts = torch.full((6,), -7, dtype=torch.int64, device=DEV)
        td, pd = _dev(t), _dev(p)
        check(lib().hdf_op_mask_flags(ptr(td), ptr(pd), k, *shape, ptr(flags), ptr(counts), st()), "hdf_op_mask_flags")
        got, cnt = flags.cpu().numpy(), counts.cpu().tolist()
        assert (got[v:] == 0xEE).all() and cnt[5] == -7, kind
        bad = np.argwhere(got[:v].reshape(shape) != ref["flags"])
        assert len(bad) == 0, (kind, len(bad), bad[:4].tolist())
        assert cnt[:5] == ref["counts"], (kind, cnt, ref["counts"])


@pytest.mark.parametrize("shape", sr.SHAPES, ids=IDS)
def test_edt_sq_every_voxel_for_both_seed_sets(shape):
    ws = _workspace(shape)
    for kind in ("blobs", "faces", "corners", "empty_t"):
        ref = sr.case_ref(shape, kind)
        flags = _dev(ref["flags"])
        for bit, want in ((sr.B26_T, ref["d2T"]), (sr.B26_P, ref["d2P"])):
            got = _edt(flags, bit, shape, ws)
            bad = np.argwhere(got != want)
            assert len(bad) == 0, (kind, bit, len(bad), bad[:4].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])
    # seed sets of the transform's own: a single seed, none (every voxel the sentinel), seeds on one face only; the other
    # bits of the byte are set everywhere and must not count
    for name, seed in sr.seed_sets(shape).items():
        flags = _dev((seed * 32 + 0xC3).astype(np.uint8))
        got, want = _edt(flags, 32, shape, ws), sr.d2_of(seed)
        if name == "none":
            assert (want == sr.NO_SEED).all()
        bad = np.argwhere(got != want)
        assert len(bad) == 0, (name, len(bad), bad[:4].tolist())
    # a mask of two bits seeds from either
    ref = sr.case_ref(shape, "blobs")
    both = (ref["flags"] & (sr.B26_T | sr.B26_P)) != 0
    assert np.array_equal(_edt(_dev(ref["flags"]), sr.B26_T | sr.B26_P, shape, ws), sr.d2_of(both))


@pytest.mark.parametrize("shape", sr.SHAPES, ids=IDS)
def test_surface_distances_histogram_result_and_floats(shape):
    """one workspace for all nine calls: each sees the histogram, the counts and the maximum of the call before it unless
    they are cleared"""
    from hdf_rt import cal_score
    from hdf_rt.surface import scores_from_result
    ws = _workspace(shape)
    for kind in sr.MASKS:
        t, p, k = sr.case(shape, kind)
        ref = sr.case_ref(shape, kind)
        td, pd = _dev(t), _dev(p)
        res, hist = _distances(td, pd, k, shape, ws)
        assert res == ref["result"], (kind, res, ref["result"])
        bad = np.argwhere(hist != ref["hist"])
        assert len(bad) == 0, (kind, len(bad), bad[:4].tolist())
        if ref["result"][11]:
            assert hist.sum() == res[6] == res[3] + res[4]
        want = sr.scores(ref["result"])
        for got in (scores_from_result(res), cal_score(pd == k, td == k), cal_score(p == k, t == k)):
            assert sorted(got) == sorted(want)
            for key, w in want.items():
                if np.isnan(w):
                    assert np.isnan(got[key]), (kind, key, got[key])
                else:
                    assert abs(got[key] - w) <= 1e-12 * abs(w), (kind, key, got[key], w)
        assert np.isnan(want["HausdorffDistance"]) == (kind in ("empty_t", "empty_p", "empty_both", "full")
                                                        or shape == (1, 1, 1))


def test_second_call_on_a_workspace_does_not_see_the_first():
    shape = (19, 67, 131)
    ws = _workspace(shape)
    seq = ["faces", "corners", "faces", "empty_both", "blobs"]
    for kind in seq:
        t, p, k = sr.case(shape, kind)
        res, hist = _distances(_dev(t), _dev(p), k, shape, ws, extra=0)
        assert res == sr.case_ref(shape, kind)["result"] and np.array_equal(hist, sr.case_ref(shape, kind)["hist"]), kind


def test_corner_voxels_give_the_diagonal():
    for shape in sr.SHAPES[1:]:
        t, p, k = sr.case(shape, "corners")
        res, hist = _distances(_dev(t), _dev(p), k, shape, _workspace(shape))
        diag = sum((s - 1) ** 2 for s in shape)
        assert res == [1, 1, 0, 1, 1, diag, 2, diag, diag, 0, 95, 1], (shape, res)
        assert hist[diag] == 2 and hist.sum() == 2
    assert sum((s - 1) ** 2 for s in (1024, 2, 3)) == 1046534


def _same(a, b):
    np.testing.assert_array_equal(np.asarray(a[0], np.float64), np.asarray(b[0], np.float64))
    np.testing.assert_array_equal(np.float64(a[1]), np.float64(b[1]))


@pytest.mark.parametrize("num_classes", [3, 4])
def test_multi_wrappers_three_labels(num_classes):
    """(40,48,56), labels 0..3; with num_classes = 4 the last class is empty on both sides: NaN there and in the mean, like
    the reference's np.mean over a list that holds a NaN"""
    from hdf_rt import multi_dice, multi_hd, multi_jc, multi_vs, surface
    shape = (40, 48, 56)
    t, p = sr.label_maps(shape, 3, 3)
    per = [sr.scores(sr.surface(t, p, k)["result"]) for k in range(1, num_classes + 1)]
    for fn, key in ((multi_dice, "Dice"), (multi_hd, "HausdorffDistance95"), (multi_vs, "VolumeSimilarity"),
                    (multi_jc, "Jaccard")):
        vals = [round(s[key], 4) for s in per]
        want = (vals, round(np.mean(vals), 4))
        _same(fn(t, p, num_classes), want)                       # numpy arrays, uploaded
        _same(fn(_dev(t), _dev(p), num_classes), want)           # device tensors, as sliding_window_predict returns
        assert np.isnan(want[1]) == (num_classes == 4)
    assert sum(1 for key in surface._workspaces if key[-3:] == shape) == 1      # one workspace per volume shape


def test_refused_arguments_launch_nothing_on_the_device():
    from hdf_rt import HdfError, multi_hd
    t = torch.zeros((4, 5, 6), dtype=torch.uint8, device=DEV)
    res = torch.full((12,), -7, dtype=torch.int64, device=DEV)
    ws = _workspace((4, 5, 6))
    assert lib().hdf_surface_distances(ptr(t), ptr(t), 0, 4, 5, 6, ptr(ws), ws.numel(), ptr(res), None, 0, st()) == 1
    assert lib().hdf_surface_distances(ptr(t), ptr(t), 1, 4, 5, 6, ptr(ws), ws.numel() - 1, ptr(res), None, 0, st()) == 1
    assert lib().hdf_last_error().startswith(b"surface:")
    assert res.cpu().tolist() == [-7] * 12
    with pytest.raises(HdfError):
        multi_hd(torch.zeros((1, 4, 1025), dtype=torch.uint8, device=DEV), torch.zeros((1, 4, 1025), dtype=torch.uint8,
                                                                                       device=DEV), 1)
