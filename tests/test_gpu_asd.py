"""The average surface distance on the device (csrc/surface_asd.hip, hdf_rt/surface.py) against the integer restatement of
the definitions in include/hdf.h (tests/asd_ref.py, itself held to MONAI's scipy call sequence and to brute force by
tests/test_asd_ref_cpu.py).

Shapes and masks are tests/surface_ref.py's, as tests/test_gpu_surface.py uses them: they are the smallest that reach
every edge of the shared distance transform and of the gather's tiling -- (1,1,1) and a depth-1 plane (all edge); odd sizes
across a wave and a tile; a 300-voxel line; the cap of 1024 on each axis in turn; (2,600,5); (40,48,56) with three labels.
The nine masks include blobs that run into the volume's faces (where E6 and C6 differ), a mask that fills the volume (its
edge is the shell) and the three empty cases (NaN / +inf).  The histogram spans up to 1 046 535 bins at the 1024 shapes:
256 workgroups of the partial sum per direction and one chain of the final kernel.

Every comparison is exact -- each flag byte, both counts, each int32 of both distance maps, every bin of both histograms --
except the two fp64 sums and the floats made from them: 1e-12 relative to math.fsum (the kernels add at most 16 + 3 terms
in a chain below two trees of depth 8: (chain + depth + 2) 2^-53 is far below it; the fp64 square root and the
product add one rounding each).  NaN and inf are checked as such, never through a tolerance.  Outputs are pre-filled with
a marker and carry a guard tail; the workspace is filled with 0x5A and reused across all masks of a shape."""
import math
import struct

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import asd_ref as ar  # noqa: E402
import surface_ref as sr  # noqa: E402
from hdf_rt._lib import check, lib, ptr  # noqa: E402
from hip_util import DEV, st  # noqa: E402

IDS = ["x".join(map(str, s)) for s in sr.SHAPES]
GUARD = 64
TOL = 1e-12


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _workspace(shape):
    n = lib().hdf_surface_asd_workspace_bytes(*shape)
    assert n > 0
    return torch.full((n,), 0x5A, dtype=torch.uint8, device=DEV)


def _f64(bits):
    return struct.unpack("<d", struct.pack("<q", bits))[0]


def _asd(t, p, k, shape, ws, extra=5):
    """(result[4] python ints, histA, histB) of one hdf_surface_asd call, guards checked"""
    nb = sr.hist_bins(shape)
    n = nb + extra
    res = torch.full((5,), -7, dtype=torch.int64, device=DEV)
    hist = torch.full((2 * n + GUARD,), 0xABCD, dtype=torch.int32, device=DEV)
    check(lib().hdf_surface_asd(ptr(t), ptr(p), k, *shape, ptr(ws), ws.numel(), ptr(res), ptr(hist), n, st()),
          "hdf_surface_asd")
    res, hist = res.cpu().tolist(), hist.cpu().numpy().astype(np.int64)
    assert res[4] == -7 and (hist[2 * n:] == 0xABCD).all(), "write past the end of an output"
    rows = hist[:2 * n].reshape(2, n)
    assert (rows[:, nb:] == 0).all(), "entries past the last possible squared distance are 0"
    return res[:4], rows[0, :nb], rows[1, :nb]


def _close(got, want):
    return got == want if want == 0 else abs(got - want) <= TOL * abs(want)


@pytest.mark.parametrize("shape", sr.SHAPES, ids=IDS)
def test_edge_flags_every_byte_and_both_counts(shape):
    v = int(np.prod(shape))
    for kind in sr.MASKS:
        t, p, k = sr.case(shape, kind)
        ref = ar.case_ref(shape, kind)
        flags = torch.full((v + GUARD,), 0xEE, dtype=torch.uint8, device=DEV)
        counts = torch.full((3,), -7, dtype=torch.int64, device=DEV)
        td, pd = _dev(t), _dev(p)
        check(lib().hdf_op_edge_flags(ptr(td), ptr(pd), k, *shape, ptr(flags), ptr(counts), st()), "hdf_op_edge_flags")
        got, cnt = flags.cpu().numpy(), counts.cpu().tolist()
        assert (got[v:] == 0xEE).all() and cnt[2] == -7, kind
        bad = np.argwhere(got[:v].reshape(shape) != ref["flags"])
        assert len(bad) == 0, (kind, len(bad), bad[:4].tolist())
        assert cnt[:2] == ref["counts"], (kind, cnt, ref["counts"])
        # beside hdf_op_mask_flags: the same two membership bits, and no other bit in common
        mflags = torch.full((v,), 0xEE, dtype=torch.uint8, device=DEV)
        mcounts = torch.zeros((5,), dtype=torch.int64, device=DEV)
        check(lib().hdf_op_mask_flags(ptr(td), ptr(pd), k, *shape, ptr(mflags), ptr(mcounts), st()), "hdf_op_mask_flags")
        mgot = mflags.cpu().numpy()
        assert np.array_equal(mgot, sr.case_ref(shape, kind)["flags"].ravel()), kind
        assert (((got[:v] ^ mgot) & 3) == 0).all() and ((got[:v] & 0x3C) == 0).all() and ((mgot & 0xC0) == 0).all(), kind


@pytest.mark.parametrize("shape", sr.SHAPES, ids=IDS)
def test_edt_sq_from_either_edge_set(shape):
    """hdf_op_edt_sq, unchanged, seeded from bits 64 and 128 of the edge flags, on a workspace of the ASD size"""
    v = int(np.prod(shape))
    ws = _workspace(shape)
    for kind in ("blobs", "faces", "corners", "empty_t", "full"):
        ref = ar.case_ref(shape, kind)
        flags = _dev(ref["flags"])
        for bit, want in ((ar.E6_T, ref["d2ET"]), (ar.E6_P, ref["d2EP"])):
            d2 = torch.full((v + GUARD,), -77, dtype=torch.int32, device=DEV)
            check(lib().hdf_op_edt_sq(ptr(flags), bit, *shape, ptr(d2), ptr(ws), ws.numel(), st()), "hdf_op_edt_sq")
            out = d2.cpu().numpy()
            assert (out[v:] == -77).all(), "write past the end of d2"
            got = out[:v].reshape(shape).astype(np.int64)
            bad = np.argwhere(got != want)
            assert len(bad) == 0, (kind, bit, len(bad), bad[:4].tolist())
        if kind == "empty_t":
            assert (ref["d2ET"] == sr.NO_SEED).all()


@pytest.mark.parametrize("shape", sr.SHAPES, ids=IDS)
def test_surface_asd_counts_histograms_sums_and_floats(shape):
    """one workspace for all nine masks: each call sees the counts and both histograms of the one before unless they are
    cleared"""
    from hdf_rt import asd_from_result, asd_scores, cal_asd
    ws = _workspace(shape)
    for kind in sr.MASKS:
        t, p, k = sr.case(shape, kind)
        ref = ar.case_ref(shape, kind)
        td, pd = _dev(t), _dev(p)
        res, hA, hB = _asd(td, pd, k, shape, ws)
        assert res[:2] == ref["counts"], (kind, res, ref["counts"])
        for name, got, want in (("A", hA, ref["histA"]), ("B", hB, ref["histB"])):
            bad = np.argwhere(got != want)
            assert len(bad) == 0, (kind, name, len(bad), bad[:4].tolist())
        if res[0] and res[1]:
            assert hA.sum() == res[1] and hB.sum() == res[0], kind           # |A| = |E6(P)|, |B| = |E6(T)|
        else:
            assert hA.sum() == 0 and hB.sum() == 0 and res[2] == 0 and res[3] == 0, (kind, res)
        sA, sB = _f64(res[2]), _f64(res[3])
        print(shape, kind, "sumA", sA, ref["sumA"], "sumB", sB, ref["sumB"])
        assert _close(sA, ref["sumA"]) and _close(sB, ref["sumB"]), (kind, sA, ref["sumA"], sB, ref["sumB"])
        again, _, _ = _asd(td, pd, k, shape, ws, extra=0)
        assert again == res, (kind, again, res)                             # the same 32 bytes
        want = ref["scores"]
        nan_keys = {key for key, w in want.items() if math.isnan(w)}
        inf_keys = {key for key, w in want.items() if math.isinf(w)}
        forms = [asd_from_result(res), asd_scores(td, pd, [k])[0], asd_scores(t, p, [k])[0]]
        for got in forms:
            assert sorted(got) == sorted(want)
            for key, w in want.items():
                if key in nan_keys:
                    assert math.isnan(got[key]), (kind, key, got[key])
                elif key in inf_keys:
                    assert math.isinf(got[key]) and got[key] > 0, (kind, key, got[key])
                else:
                    assert _close(got[key], w), (kind, key, got[key], w)
        # cal_asd(predict, target): device tensors, numpy, and the reference's [1, 1, a, b, c] boolean form
        for got in (cal_asd(pd == k, td == k), cal_asd((p == k).astype(np.uint8), (t == k).astype(np.uint8)),
                    cal_asd(torch.from_numpy(p == k)[None, None], torch.from_numpy(t == k)[None, None]),
                    cal_asd((p == k)[None, None], (t == k)[None, None])):
            assert isinstance(got, float)
            if "ASD" in nan_keys:
                assert math.isnan(got), (kind, got)
            elif "ASD" in inf_keys:
                assert math.isinf(got) and got > 0, (kind, got)
            else:
                assert _close(got, want["ASD"]), (kind, got, want["ASD"])
        if shape != (1, 1, 1):      # (a single voxel is in a mask or not: the seeded kinds are what they happen to be)
            assert ("ASD" in nan_keys) == (kind == "empty_both") and ("ASD" in inf_keys) == (kind in ("empty_t", "empty_p"))


def test_second_call_on_a_workspace_does_not_see_the_first():
    shape = (19, 67, 131)
    ws = _workspace(shape)
    for kind in ["faces", "corners", "faces", "empty_both", "full", "empty_p", "blobs"]:
        t, p, k = sr.case(shape, kind)
        ref = ar.case_ref(shape, kind)
        res, hA, hB = _asd(_dev(t), _dev(p), k, shape, ws, extra=0)
        assert res[:2] == ref["counts"] and np.array_equal(hA, ref["histA"]) and np.array_equal(hB, ref["histB"]), kind
        assert _close(_f64(res[2]), ref["sumA"]) and _close(_f64(res[3]), ref["sumB"]), kind


def test_corner_voxels_give_the_diagonal():
    for shape in sr.SHAPES[1:]:
        t, p, k = sr.case(shape, "corners")
        res, hA, hB = _asd(_dev(t), _dev(p), k, shape, _workspace(shape))
        diag = sum((s - 1) ** 2 for s in shape)
        assert res[:2] == [1, 1] and hA[diag] == 1 and hB[diag] == 1 and hA.sum() == 1 and hB.sum() == 1, (shape, res)
        assert _f64(res[2]) == math.sqrt(diag) and _f64(res[3]) == math.sqrt(diag), (shape, res)


def _same(a, b):
    np.testing.assert_array_equal(np.asarray(a[0], np.float64), np.asarray(b[0], np.float64))
    np.testing.assert_array_equal(np.float64(a[1]), np.float64(b[1]))


@pytest.mark.parametrize("num_classes", [3, 4])
def test_multi_asd_three_labels(num_classes):
    """(40,48,56), labels 0..3; with num_classes = 4 the last class is empty on both sides: NaN there and in the mean, like
    the reference's np.mean over a list that holds a NaN"""
    from hdf_rt import asd_scores, multi_asd, surface
    shape = (40, 48, 56)
    t, p = sr.label_maps(shape, 3, 3)
    per = [ar.asd(t, p, k)["scores"] for k in range(1, num_classes + 1)]
    vals = [round(s["ASD"], 4) for s in per]
    want = (vals, round(np.mean(vals), 4))
    assert all(math.isfinite(v) and v > 0 for v in vals[:3]) and math.isnan(want[1]) == (num_classes == 4)
    _same(multi_asd(t, p, num_classes), want)                       # numpy arrays, uploaded
    _same(multi_asd(_dev(t), _dev(p), num_classes), want)           # device tensors, as sliding_window_predict returns
    rows = asd_scores(_dev(t), _dev(p), range(1, num_classes + 1))  # all classes enqueued, one copy back
    for got, w in zip(rows, per):
        for key in w:
            assert ar.same_float(got[key], w[key], TOL), (key, got[key], w[key])
    assert sum(1 for key in surface._asd_workspaces if key[-3:] == shape) == 1      # one workspace per volume shape
    assert not any(key[-3:] == shape and ws.numel() != lib().hdf_surface_workspace_bytes(*shape)
                   for key, ws in surface._workspaces.items())      # and never in the cal_score cache
    surface.clear_workspaces()
    assert not surface._asd_workspaces and not surface._workspaces


def test_refused_arguments_launch_nothing_on_the_device():
    from hdf_rt import HdfError, multi_asd
    shape = (4, 5, 6)
    t = torch.zeros(shape, dtype=torch.uint8, device=DEV)
    res = torch.full((4,), -7, dtype=torch.int64, device=DEV)
    flags = torch.full((120,), 0xEE, dtype=torch.uint8, device=DEV)
    hist = torch.full((2 * 8,), 0xABCD, dtype=torch.int32, device=DEV)
    ws = _workspace(shape)
    f = lib().hdf_surface_asd
    calls = [f(ptr(t), ptr(t), 1, 0, 5, 6, ptr(ws), ws.numel(), ptr(res), ptr(hist), 8, st()),
             f(ptr(t), ptr(t), 1, 4, 5, 1025, ptr(ws), 1 << 40, ptr(res), ptr(hist), 8, st()),
             f(ptr(t), ptr(t), 0, 4, 5, 6, ptr(ws), ws.numel(), ptr(res), ptr(hist), 8, st()),
             f(ptr(t), ptr(t), 256, 4, 5, 6, ptr(ws), ws.numel(), ptr(res), ptr(hist), 8, st()),
             f(ptr(t), ptr(t), 1, 4, 5, 6, ptr(ws), ws.numel() - 1, ptr(res), ptr(hist), 8, st()),
             f(ptr(t), ptr(t), 1, 4, 5, 6, ptr(ws), ws.numel(), ptr(res), ptr(hist), -1, st())]
    for rc in calls:
        assert rc == 1
    assert lib().hdf_last_error().startswith(b"surface:")
    g = lib().hdf_op_edge_flags
    for rc in (g(ptr(t), ptr(t), 1, 0, 5, 6, ptr(flags), ptr(res), st()), g(ptr(t), ptr(t), 1, 4, 1025, 6, ptr(flags), ptr(res), st()),
               g(ptr(t), ptr(t), 0, 4, 5, 6, ptr(flags), ptr(res), st()), g(ptr(t), ptr(t), 256, 4, 5, 6, ptr(flags), ptr(res), st())):
        assert rc == 1 and lib().hdf_last_error().startswith(b"surface:")
    assert lib().hdf_surface_asd_workspace_bytes(1025, 1, 1) == -1
    torch.cuda.synchronize()
    assert res.cpu().tolist() == [-7] * 4 and (flags.cpu() == 0xEE).all() and (hist.cpu() == 0xABCD).all()
    assert (ws.cpu() == 0x5A).all()
    with pytest.raises(HdfError):
        multi_asd(torch.zeros((1, 4, 1025), dtype=torch.uint8, device=DEV), torch.zeros((1, 4, 1025), dtype=torch.uint8,
                                                                                        device=DEV), 1)
