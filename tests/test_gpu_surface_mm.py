"""Surface distances in physical units on the device (csrc/surface_mm.hip, hdf_rt/surface.py with spacing=) against the fp64
restatement of the definitions in include/hdf.h (tests/surface_mm_ref.py, itself held to brute force in every bit by
tests/test_surface_mm_ref_cpu.py).

Shapes (surface_ref.SHAPES): (1,1,1) and a depth-1 volume; (19,67,131), odd and across a wave and a tile on every axis;
(5,3,300); the cap of 1024 on each axis in turn (LDS tiles of 4 fp64 lines, and +inf lines beside real ones in the corners
case) and (2,600,5) (tiles of 8); the transform alone also at (3,300,9), the one tile width (16) the others do not reach.
Spacings (surface_mm_ref.SPACINGS): unit, thick slices along either end axis, one whose weights are not representable,
(2.5,1,1); (19,67,131) takes two of them.

Compared in every bit: each fp64 of both distance maps, the twelve result words, both outputs of hdf_op_select_u64 on the
crafted key sets.  The two ASD sums: 1e-12 relative to math.fsum -- the bound the unit-spacing sums are held to; a sum of n
terms in any order is within (n - 1) 2^-53 relative, 1e-12 up to 9000 terms a chain, and no chain here is longer than a
thread's share of 4096 voxels plus a tree -- and the same bits on a second call.  The wrappers' floats: 1e-12 relative to
the restatement's, NaN and +inf exactly where the definitions say.  Outputs are pre-filled with a marker and carry a guard
tail; one workspace per shape, pre-filled with 0x5A, serves every mask, spacing and entry without being cleared."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import asd_ref as ar  # noqa: E402
import surface_mm_ref as mm  # noqa: E402
import surface_ref as sr  # noqa: E402
from hdf_rt._lib import check, lib, ptr  # noqa: E402
from hip_util import DEV, st  # noqa: E402

SHAPES = [s for s in sr.SHAPES if s != (40, 48, 56)]
IDS = ["x".join(map(str, s)) for s in SHAPES]
GUARD = 64
MARK = -77.0


def _spacings(shape):
    return [mm.SPACINGS[3], mm.SPACINGS[1]] if shape == (19, 67, 131) else mm.SPACINGS


def _sp(s):
    return (C.c_double * 3)(*s)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _workspace(shape):
    n = lib().hdf_surface_mm_workspace_bytes(*shape)
    assert n > 0
    return torch.full((n,), 0x5A, dtype=torch.uint8, device=DEV)


def _edt(flags, seed_bit, shape, spacing, ws):
    v = int(np.prod(shape))
    d2 = torch.full((v + GUARD,), MARK, dtype=torch.float64, device=DEV)
    check(lib().hdf_op_edt_sq_mm(ptr(flags), seed_bit, *shape, _sp(spacing), ptr(d2), ptr(ws), ws.numel(), st()),
          "hdf_op_edt_sq_mm")
    out = d2.cpu().numpy()
    assert (out[v:] == MARK).all(), "write past the end of d2"
    return out[:v].reshape(shape)


def _same_bits(got, want, what):
    bad = np.argwhere(got.view(np.uint64) != want.view(np.uint64))
    assert len(bad) == 0, (what, len(bad), bad[:4].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


def _distances(t, p, k, shape, spacing, ws):
    res = torch.full((13,), -7, dtype=torch.int64, device=DEV)
    check(lib().hdf_surface_distances_mm(ptr(t), ptr(p), k, *shape, _sp(spacing), ptr(ws), ws.numel(), ptr(res), st()),
          "hdf_surface_distances_mm")
    res = res.cpu().tolist()
    assert res[12] == -7, "write past the end of result"
    return [v & 0xFFFFFFFFFFFFFFFF for v in res[:12]]


def _asd(t, p, k, shape, spacing, ws):
    res = torch.full((5,), -7, dtype=torch.int64, device=DEV)
    check(lib().hdf_surface_asd_mm(ptr(t), ptr(p), k, *shape, _sp(spacing), ptr(ws), ws.numel(), ptr(res), st()),
          "hdf_surface_asd_mm")
    res = res.cpu().tolist()
    assert res[4] == -7, "write past the end of result"
    return [v & 0xFFFFFFFFFFFFFFFF for v in res[:4]]


def _close(got, want, rel=1e-12):
    return ar.same_float(got, want, rel)


@pytest.mark.parametrize("shape", SHAPES + [(3, 300, 9)], ids=IDS + ["3x300x9"])
def test_edt_sq_mm_every_voxel_in_every_bit(shape):
    ws = _workspace(shape)
    if shape == (3, 300, 9):                                  # not one of surface_ref's cases: seed sets of its own
        for spacing in (mm.SPACINGS[3], mm.SPACINGS[1]):
            for name, seed in sr.seed_sets(shape).items():
                got = _edt(_dev((seed * 4 + 0xC3).astype(np.uint8)), 4, shape, spacing, ws)
                _same_bits(got, mm.d2_mm(seed, spacing), (name, spacing))
        return
    for spacing in _spacings(shape):
        for kind in ("blobs", "faces", "corners", "empty_t"):
            ref = mm.case_ref(shape, kind, spacing)
            flags = _dev(ref["flags"])
            for bit, key in ((sr.B26_T, "d2T"), (sr.B26_P, "d2P")):
                _same_bits(_edt(flags, bit, shape, spacing, ws), ref[key], (kind, spacing, key))
    # seed sets of the transform's own: a single seed, none (every voxel +inf), seeds on one face only; the other bits of
    # the byte are set everywhere and must not count
    spacing = _spacings(shape)[0]
    for name, seed in sr.seed_sets(shape).items():
        got = _edt(_dev((seed * 32 + 0xC3).astype(np.uint8)), 32, shape, spacing, ws)
        if name == "none":
            assert np.isposinf(got).all()
        _same_bits(got, mm.d2_mm(seed, spacing), (name, spacing))


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_surface_distances_mm_result_words_and_floats(shape):
    """one workspace for every mask and spacing: each call sees the counts, the maximum and the select's state of the call
    before it unless they are cleared"""
    from hdf_rt import cal_score
    from hdf_rt.surface import scores_from_result_mm
    ws = _workspace(shape)
    for spacing in _spacings(shape):
        for kind in sr.MASKS:
            t, p, k = sr.case(shape, kind)
            ref = mm.case_ref(shape, kind, spacing)
            td, pd = _dev(t), _dev(p)
            res = _distances(td, pd, k, shape, spacing, ws)
            assert res == ref["result"], (kind, spacing, res, ref["result"])
            if not res[11]:
                assert res[5:11] == [0] * 6
            want = mm.scores(ref["result"])
            for got in (scores_from_result_mm(res), cal_score(pd == k, td == k, spacing=spacing)):
                assert sorted(got) == sorted(want)
                for key, w in want.items():
                    assert _close(got[key], w), (kind, spacing, key, got[key], w)
            assert np.isnan(want["HausdorffDistance"]) == (kind in ("empty_t", "empty_p", "empty_both", "full")
                                                            or shape == (1, 1, 1))


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_surface_asd_mm_counts_sums_and_floats(shape):
    from hdf_rt import asd_from_result, cal_asd
    ws = _workspace(shape)
    for spacing in _spacings(shape):
        for kind in sr.MASKS:
            t, p, k = sr.case(shape, kind)
            ref = mm.asd_case_ref(shape, kind, spacing)
            td, pd = _dev(t), _dev(p)
            res = _asd(td, pd, k, shape, spacing, ws)
            assert res[:2] == ref["counts"], (kind, spacing, res, ref["counts"])
            sums = [mm.unbits(res[2]), mm.unbits(res[3])]
            for got, want in zip(sums, (ref["sumA"], ref["sumB"])):
                assert abs(got - want) <= 1e-12 * abs(want), (kind, spacing, got, want)
            if not (res[0] and res[1]):
                assert res[2:] == [0, 0]                      # +0, both
            assert _asd(td, pd, k, shape, spacing, ws) == res, (kind, spacing)      # the same bits on a second call
            signed = [v - (1 << 64) if v >> 63 else v for v in res]
            for got in (asd_from_result(signed), ):
                for key, w in ref["scores"].items():
                    assert _close(got[key], w), (kind, spacing, key, got[key], w)
            assert _close(cal_asd(pd == k, td == k, spacing=spacing), ref["scores"]["ASD"]), (kind, spacing)
            n_t, n_p = ref["counts"]
            sym = ref["scores"]["ASD"]
            assert math.isnan(sym) == (n_t == 0 and n_p == 0) and math.isinf(sym) == ((n_t == 0) != (n_p == 0))


def test_select_u64_on_the_crafted_key_sets():
    ws = torch.full((49408 + GUARD,), 0x5A, dtype=torch.uint8, device=DEV)
    for name, keys, ranks in mm.select_cases():
        kd = _dev(keys.view(np.int64))
        for lo in ranks:
            out = torch.full((3,), -7, dtype=torch.int64, device=DEV)
            check(lib().hdf_op_select_u64(ptr(kd), len(keys), lo, ptr(ws), 49408, ptr(out), st()), "hdf_op_select_u64")
            got = out.cpu().tolist()
            assert got[2] == -7, "write past the end of out2"
            assert tuple(v & 0xFFFFFFFFFFFFFFFF for v in got[:2]) == mm.select_ref(keys, lo), (name, lo)
    assert (ws[49408:].cpu().numpy() == 0x5A).all(), "write past the end of the select's workspace"


def test_unit_spacing_equals_the_integer_entries_on_the_device():
    """the same inputs through hdf_surface_distances / hdf_surface_asd and through the _mm entries at (1, 1, 1): counts,
    hd2, S[lo] and S[hi] are equal as numbers"""
    one = (1.0, 1.0, 1.0)
    for shape in ((19, 67, 131), (2, 3, 1024), (2, 600, 5)):
        ws = _workspace(shape)
        n_int = lib().hdf_surface_asd_workspace_bytes(*shape)
        ws_int = torch.full((n_int,), 0x5A, dtype=torch.uint8, device=DEV)
        for kind in sr.MASKS:
            t, p, k = sr.case(shape, kind)
            td, pd = _dev(t), _dev(p)
            res = torch.full((12,), -7, dtype=torch.int64, device=DEV)
            check(lib().hdf_surface_distances(ptr(td), ptr(pd), k, *shape, ptr(ws_int), n_int, ptr(res), None, 0, st()),
                  "hdf_surface_distances")
            want, got = res.cpu().tolist(), _distances(td, pd, k, shape, one, ws)
            for w in (5, 7, 8):
                x = mm.unbits(got[w])
                assert x == int(x)
                got[w] = int(x)
            assert got == want, (shape, kind, got, want)
            res4 = torch.full((4,), -7, dtype=torch.int64, device=DEV)
            check(lib().hdf_surface_asd(ptr(td), ptr(pd), k, *shape, ptr(ws_int), n_int, ptr(res4), None, 0, st()),
                  "hdf_surface_asd")
            want, got = res4.cpu().tolist(), _asd(td, pd, k, shape, one, ws)
            assert got[:2] == want[:2], (shape, kind)
            for a, b in zip(got[2:], want[2:]):
                assert abs(mm.unbits(a) - mm.unbits(b)) <= 1e-12 * abs(mm.unbits(b)), (shape, kind)


def _same(a, b):
    np.testing.assert_array_equal(np.asarray(a[0], np.float64), np.asarray(b[0], np.float64))
    np.testing.assert_array_equal(np.float64(a[1]), np.float64(b[1]))


@pytest.mark.parametrize("num_classes", [3, 4])
def test_multi_wrappers_with_a_spacing(num_classes):
    """(12,20,28), labels 0..3; with num_classes = 4 the last class is empty on both sides: NaN there and in the mean"""
    from hdf_rt import (asd_scores, multi_asd, multi_dice, multi_hd, multi_jc, multi_vs, surface, surface_scores)
    shape, spacing = (12, 20, 28), (3.0, 0.5, 0.5)
    t, p = sr.label_maps(shape, 3, 3)
    per = [mm.scores(mm.surface(t, p, k, spacing)["result"]) for k in range(1, num_classes + 1)]
    surface.clear_workspaces()
    for fn, key in ((multi_dice, "Dice"), (multi_hd, "HausdorffDistance95"), (multi_vs, "VolumeSimilarity"),
                    (multi_jc, "Jaccard")):
        vals = [round(s[key], 4) for s in per]
        want = (vals, round(np.mean(vals), 4))
        _same(fn(t, p, num_classes, spacing=spacing), want)                    # numpy arrays, uploaded
        _same(fn(_dev(t), _dev(p), num_classes, spacing=spacing), want)        # device tensors
        assert np.isnan(want[1]) == (num_classes == 4)
    got = surface_scores(t, p, range(1, num_classes + 1), spacing=spacing)
    for g, w in zip(got, per):
        for key in w:
            assert _close(g[key], w[key]), (key, g[key], w[key])
    aper = [mm.asd(t, p, k, spacing)["scores"] for k in range(1, num_classes + 1)]
    vals = [round(s["ASD"], 4) for s in aper]
    _same(multi_asd(_dev(t), _dev(p), num_classes, spacing=spacing), (vals, round(np.mean(vals), 4)))
    for g, w in zip(asd_scores(t, p, range(1, num_classes + 1), spacing=spacing), aper):
        for key in w:
            assert _close(g[key], w[key]), (key, g[key], w[key])
    # the anisotropy is seen: the unit-spacing numbers differ
    assert multi_hd(t, p, 3)[0] != multi_hd(t, p, 3, spacing=spacing)[0]
    # one workspace per volume shape for both entries, in a cache of its own that clear_workspaces() empties too
    assert sum(1 for key in surface._mm_workspaces if key[-3:] == shape) == 1
    surface.clear_workspaces()
    assert not surface._mm_workspaces and not surface._workspaces and not surface._asd_workspaces


def test_refused_arguments_launch_nothing_on_the_device():
    from hdf_rt import HdfError, cal_asd, multi_hd
    shape = (4, 5, 6)
    t = torch.ones(shape, dtype=torch.uint8, device=DEV)
    t[0] = 0
    res = torch.full((12,), -7, dtype=torch.int64, device=DEV)
    d2 = torch.full((120,), MARK, dtype=torch.float64, device=DEV)
    ws = _workspace(shape)
    ok, L = _sp((1.0, 2.0, 3.0)), lib()
    calls = [lambda sp, k, n: L.hdf_surface_distances_mm(ptr(t), ptr(t), k, *shape, sp, ptr(ws), n, ptr(res), st()),
             lambda sp, k, n: L.hdf_surface_asd_mm(ptr(t), ptr(t), k, *shape, sp, ptr(ws), n, ptr(res), st()),
             lambda sp, k, n: L.hdf_op_edt_sq_mm(ptr(t), k, *shape, sp, ptr(d2), ptr(ws), n, st())]
    for call in calls:
        for sp in (None, _sp((0.0, 1, 1)), _sp((1, float("nan"), 1)), _sp((1, 1, 2048.0)), _sp((1, -1.0, 1))):
            assert call(sp, 1, ws.numel()) == 1 and b"spacing" in L.hdf_last_error()
        assert call(ok, 0, ws.numel()) == 1 and L.hdf_last_error().startswith(b"surface:")
        assert call(ok, 1, ws.numel() - 1) == 1 and b"workspace" in L.hdf_last_error()
    keys = torch.arange(10, dtype=torch.int64, device=DEV)
    for n, lo, nbytes in ((0, 0, 49408), (10, 10, 49408), (10, -1, 49408), (10, 3, 49407)):
        assert L.hdf_op_select_u64(ptr(keys), n, lo, ptr(ws), nbytes, ptr(res), st()) == 1
        assert L.hdf_last_error().startswith(b"surface:")
    torch.cuda.synchronize()
    assert res.cpu().tolist() == [-7] * 12 and (d2.cpu().numpy() == MARK).all()
    assert (ws.cpu().numpy() == 0x5A).all()
    with pytest.raises(HdfError):
        multi_hd(t, t, 1, spacing=(0.0, 1.0, 1.0))
    with pytest.raises(HdfError):
        cal_asd(t, t, spacing=(1.0, 1.0, float("inf")))
    with pytest.raises(HdfError):
        z = torch.zeros((1, 4, 1025), dtype=torch.uint8, device=DEV)
        multi_hd(z, z, 1, spacing=(1.0, 1.0, 1.0))
