"""Host-side checks of the average-surface-distance path (no GPU):
  * tests/asd_ref.py, the integer restatement the GPU tests compare against, held to the sequence of scipy calls that
    MONAI's SurfaceDistanceMetric makes (m ^ binary_erosion(m), distance_transform_edt(~e)[other], concatenate, mean)
    on every input of the GPU tests: 1e-12 relative, NaN and inf in the same places.  MONAI itself is not run: the
    sequence comes from reading its source (include/hdf.h says so);
  * the restatement against an all-pairs brute force on volumes of at most about 7x6x5, a depth-1 volume and a full mask
    among them: integers exact;
  * six planted defects (C6 edges, 26-neighbour erosion, distance to the mask, mean of the two directed means, root mean
    square, the directed value as the symmetric one): each must move the ASD by more than 1e-9 relative on inputs of
    tests/test_gpu_asd.py, so those inputs can see it;
  * the three C entries on both sides of the ABI, the four Python names, and the refusals, which happen before anything
    is launched."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch
from scipy import ndimage as ndi

import asd_ref as ar
import surface_ref as sr
from conftest import ROOT

IDS = ["x".join(map(str, s)) for s in sr.SHAPES]


# ------------------------------------------------------------------------------ the restatement against MONAI's calls
def _monai_sequence(T, P):
    """get_mask_edges + get_surface_distance + compute_average_surface_distance as scipy calls, both directions"""
    eP, eT = P ^ ndi.binary_erosion(P), T ^ ndi.binary_erosion(T)

    def distances(e_from, e_to):
        if not e_to.any():
            return np.full(int(e_from.sum()), np.inf)
        return ndi.distance_transform_edt(~e_to)[e_from]

    a, b = distances(eP, eT), distances(eT, eP)
    both = np.concatenate([a, b])
    mean = lambda v: float("nan") if v.shape == (0,) else float(v.mean())      # noqa: E731
    return {"ASD": mean(both), "ASD_pred_to_gt": mean(a), "ASD_gt_to_pred": mean(b)}


@pytest.mark.parametrize("shape", sr.SHAPES, ids=IDS)
def test_restatement_equals_the_scipy_sequence_monai_runs(shape):
    for kind in sr.MASKS:
        t, p, k = sr.case(shape, kind)
        got, want = ar.case_ref(shape, kind)["scores"], _monai_sequence(t == k, p == k)
        for key in ("ASD", "ASD_pred_to_gt", "ASD_gt_to_pred"):
            assert ar.same_float(got[key], want[key], 1e-12), (kind, key, got[key], want[key])
        # the empty sets fall where include/hdf.h says
        n_t, n_p = ar.case_ref(shape, kind)["counts"]
        assert (n_t == 0) == (not (t == k).any()) and (n_p == 0) == (not (p == k).any())
        if shape != (1, 1, 1):      # (a single voxel is in a mask or not: the seeded kinds are what they happen to be)
            assert (n_t == 0) == (kind in ("empty_t", "empty_both")) and (n_p == 0) == (kind in ("empty_p", "empty_both"))
        if n_t == 0 and n_p == 0:
            assert all(math.isnan(v) for v in got.values())
        elif n_t == 0:
            assert math.isinf(got["ASD"]) and math.isinf(got["ASD_pred_to_gt"]) and math.isnan(got["ASD_gt_to_pred"])
        elif n_p == 0:
            assert math.isinf(got["ASD"]) and math.isnan(got["ASD_pred_to_gt"]) and math.isinf(got["ASD_gt_to_pred"])
        else:
            assert all(math.isfinite(v) for v in got.values())
        if kind == "identical" and n_t:
            assert got["ASD"] == 0.0


# ---------------------------------------------------------------------------------- the restatement against brute force
OFF6 = [(-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)]


def _brute_edges(mask):
    out = np.zeros_like(mask)
    for v in zip(*np.nonzero(mask)):
        for o in OFF6:
            n = tuple(a + b for a, b in zip(v, o))
            if not all(0 <= c < s for c, s in zip(n, mask.shape)) or not mask[n]:
                out[v] = True
    return out


def _brute_d2(seed):
    pts = np.argwhere(seed)
    if len(pts) == 0:
        return np.full(seed.shape, sr.NO_SEED, np.int64)
    grid = np.indices(seed.shape).reshape(3, -1).T
    return ((grid[:, None, :] - pts[None, :, :]) ** 2).sum(-1).min(1).reshape(seed.shape)


@pytest.mark.parametrize("shape,seed,full", [((5, 6, 7), 0, False), ((7, 6, 5), 1, False), ((6, 5, 7), 2, True),
                                             ((1, 6, 7), 3, False), ((7, 1, 5), 4, False), ((1, 6, 7), 5, True)])
def test_restatement_equals_brute_force(shape, seed, full):
    t, p = sr.blobs(shape, seed, 0.3)
    if full:
        t = np.ones(shape, np.uint8)
    ref = ar.asd(t, p, 1)
    T, P = t == 1, p == 1
    eT, eP = _brute_edges(T), _brute_edges(P)
    assert np.array_equal(ref["flags"], T * 1 + P * 2 + eT * 64 + eP * 128)
    assert ref["counts"] == [eT.sum(), eP.sum()] and min(ref["counts"]) > 0
    bT, bP = _brute_d2(eT), _brute_d2(eP)
    assert np.array_equal(ref["d2ET"], bT) and np.array_equal(ref["d2EP"], bP)
    A, B = np.sort(bT[eP]), np.sort(bP[eT])
    assert np.array_equal(np.repeat(np.arange(len(ref["histA"])), ref["histA"]), A)
    assert np.array_equal(np.repeat(np.arange(len(ref["histB"])), ref["histB"]), B)
    sA, sB = math.fsum(np.sqrt(A.astype(np.float64))), math.fsum(np.sqrt(B.astype(np.float64)))
    assert abs(ref["sumA"] - sA) <= 1e-12 * sA and abs(ref["sumB"] - sB) <= 1e-12 * sB
    want = (sA + sB) / (len(A) + len(B))
    assert abs(ref["scores"]["ASD"] - want) <= 1e-12 * want
    assert abs(ref["scores"]["ASD_pred_to_gt"] - sA / len(A)) <= 1e-12 * sA / len(A)
    if shape[0] == 1:
        assert np.array_equal(eT, T) and np.array_equal(eP, P)                 # a depth-1 volume is all edge
    if full:                                                                   # the shell of the volume
        shell = np.ones(shape, bool)
        shell[tuple(slice(1, -1) for _ in shape)] = False
        assert np.array_equal(eT, shell)


def test_e6_and_c6_differ_exactly_on_the_volume_faces():
    for shape in ((19, 67, 131), (40, 48, 56)):
        t, _p, k = sr.case(shape, "faces")
        T = t == k
        diff = ar.edges(T) ^ sr.border(T, sr.S6)
        face = np.zeros(shape, bool)
        for ax in range(3):
            sl = [slice(None)] * 3
            for end in (0, -1):
                sl[ax] = end
                face[tuple(sl)] = True
        assert diff.any() and not (diff & ~face).any()


# -------------------------------------------------------------------------------------------------- planted defects
@pytest.mark.parametrize("defect", ar.DEFECTS)
def test_gpu_inputs_can_see_each_planted_defect(defect):
    for shape in ((19, 67, 131), (40, 48, 56)):
        for kind in ("blobs", "faces", "full"):
            t, p, k = sr.case(shape, kind)
            good, bad = ar.case_ref(shape, kind)["scores"]["ASD"], ar.asd(t, p, k, defect=defect)["scores"]["ASD"]
            assert math.isfinite(good) and good > 0
            assert not ar.same_float(bad, good, 1e-9), (shape, kind, defect, bad, good)


# -------------------------------------------------------------------------------------------------- the C ABI on the host
@pytest.fixture(scope="module")
def lib():
    from hdf_rt import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import importlib.util
        spec = importlib.util.spec_from_file_location("hdf_build", os.path.join(ROOT, "h-denseformer_amd", "build.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mod.build(verbose=False)
    return _lib.lib()


def test_asd_entries_are_declared_exported_and_bound(lib):
    import hdf_rt
    from hdf_rt import _lib
    hdr = " ".join(open(os.path.join(ROOT, "include", "hdf.h")).read().split())
    for name, ret, nargs in (("hdf_surface_asd_workspace_bytes", "int64_t", 3), ("hdf_op_edge_flags", "int", 9),
                             ("hdf_surface_asd", "int", 12)):
        assert name in _lib.EXPORTS and hasattr(lib, name) and f"{ret} {name}(" in hdr, name
        assert len(_lib._PROTOS[name][1]) == nargs, name
        decl = hdr[hdr.index(f"{ret} {name}("):]
        assert decl[:decl.index(")")].count(",") + 1 == nargs, name
    assert _lib._PROTOS["hdf_surface_asd_workspace_bytes"][0] is C.c_int64
    for name in ("asd_from_result", "asd_scores", "cal_asd", "multi_asd"):
        assert name in dir(hdf_rt) and callable(getattr(hdf_rt, name)), name


def test_asd_entries_refuse_bad_arguments_before_any_launch(lib):
    """HDF_ERR_ARG (1) with a "surface:" message; on a host without a device a memset or a launch would come back as
    HDF_ERR_HIP (2).  The addresses are never dereferenced."""
    buf = (C.c_uint64 * 16)()
    a = C.addressof(buf)
    big = 1 << 40

    def both(D, H, W, label, ws_bytes, hist_len=0):
        return [lib.hdf_op_edge_flags(a, a, label, D, H, W, a, a, None),
                lib.hdf_surface_asd(a, a, label, D, H, W, a, ws_bytes, a, None, hist_len, None)]

    for dims in ((0, 8, 8), (8, 0, 8), (8, 8, 0), (1025, 8, 8), (8, 1025, 8), (8, 8, 1025)):
        assert lib.hdf_surface_asd_workspace_bytes(*dims) == -1 and lib.hdf_last_error().startswith(b"surface:")
        for rc in both(*dims, 1, big):
            assert rc == 1 and lib.hdf_last_error().startswith(b"surface:"), (dims, rc, lib.hdf_last_error())
    assert lib.hdf_surface_asd_workspace_bytes(1025, 1, 1) == -1
    for label in (0, 256):
        for rc in both(8, 8, 8, label, big):
            assert rc == 1 and lib.hdf_last_error().startswith(b"surface:"), (label, rc)
    need = lib.hdf_surface_asd_workspace_bytes(8, 9, 10)
    assert need > 0
    assert lib.hdf_surface_asd(a, a, 1, 8, 9, 10, a, need - 1, a, None, 0, None) == 1
    assert lib.hdf_last_error().startswith(b"surface:")
    assert lib.hdf_surface_asd(a, a, 1, 8, 9, 10, a, need, a, None, -1, None) == 1
    assert lib.hdf_last_error().startswith(b"surface:")
    assert all(buf[i] == 0 for i in range(16))


def test_asd_workspace_serves_edt_sq(lib):
    """hdf_op_edt_sq checks its workspace against hdf_surface_workspace_bytes: the ASD size is never below it, so one
    allocation of either size serves the transform"""
    for shape in sr.SHAPES + [(144, 144, 144), (240, 240, 155), (1024, 1024, 1024)]:
        n = lib.hdf_surface_asd_workspace_bytes(*shape)
        assert n >= lib.hdf_surface_workspace_bytes(*shape) > 0 and n % 256 == 0, shape


def test_asd_wrappers_fail_loudly_without_a_device(monkeypatch):
    from hdf_rt import HdfError, asd_scores, cal_asd, multi_asd
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)     # (so that the test is the same where there is one)
    t, p = sr.label_maps((8, 9, 10), 1, 2)
    with pytest.raises(HdfError):
        multi_asd(t, p, 2)
    with pytest.raises(HdfError):
        asd_scores(torch.from_numpy(t), torch.from_numpy(p), [1])
    with pytest.raises(HdfError):
        cal_asd(p == 1, t == 1)
    with pytest.raises(HdfError):
        cal_asd((p == 1)[None, None], (t == 1)[None, None])


def test_asd_from_result_forms_nan_and_inf_from_the_counts():
    import struct

    from hdf_rt import asd_from_result
    bits = lambda x: struct.unpack("<q", struct.pack("<d", x))[0]              # noqa: E731
    s = asd_from_result([3, 5, bits(4.0), bits(2.0)])
    assert s == {"ASD": 6.0 / 8, "ASD_pred_to_gt": 4.0 / 5, "ASD_gt_to_pred": 2.0 / 3}
    s = asd_from_result([0, 0, 0, 0])
    assert all(math.isnan(v) for v in s.values())
    s = asd_from_result([0, 5, 0, 0])                                          # E6(T) empty
    assert math.isinf(s["ASD"]) and s["ASD"] > 0 and math.isinf(s["ASD_pred_to_gt"]) and math.isnan(s["ASD_gt_to_pred"])
    s = asd_from_result([5, 0, 0, 0])                                          # E6(P) empty
    assert math.isinf(s["ASD"]) and math.isnan(s["ASD_pred_to_gt"]) and math.isinf(s["ASD_gt_to_pred"])
