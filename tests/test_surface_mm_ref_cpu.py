"""Host-side checks of the physical-unit surface distances (no GPU):
  * tests/surface_mm_ref.py, the fp64 restatement the GPU tests compare against, held to a brute force over all seeds in
    EVERY BIT on volumes up to 12x11x10 for each spacing of the GPU tests (and a few whose weights are not representable),
    and to scipy's distance_transform_edt(sampling=s)**2 within 1e-12 relative;
  * with spacing (1, 1, 1) it reproduces surface_ref / asd_ref on their own cases: the maps and the result words as
    integers, the two sums to 1e-12;
  * a hand-worked case in which anisotropy changes the nearest seed;
  * six planted defects (weights on the wrong axes, spacing not squared, the nearest seed taken in voxels and then weighted,
    `hi` as the next distinct value, a rank off by one, a sum accumulated in fp32): each must change what the GPU tests
    compare, on inputs of those tests;
  * the five C entries on both sides of the ABI, every refusal that needs no device (the spacing is a host pointer and is
    checked first), and the Python names: they raise without a GPU and do not touch the new entries when spacing is None."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch
from scipy import ndimage as ndi

import asd_ref as ar
import surface_mm_ref as mm
import surface_ref as sr
from conftest import ROOT

IDS = ["x".join(map(str, s)) for s in sr.SHAPES]
EXTRA_SPACINGS = [(0.3125, 2.9, 1.3), (0.7, 0.7, 0.7), (2.9, 0.3125, 2.5)]


# ------------------------------------------------------------------------------ the restatement against brute force
@pytest.mark.parametrize("spacing", mm.SPACINGS + EXTRA_SPACINGS, ids=str)
def test_separable_passes_equal_brute_force_in_every_bit(spacing):
    rng = np.random.default_rng(int(sum(spacing) * 1000))
    shapes = [(12, 11, 10), (1, 9, 12), (7, 1, 5), (5, 6, 1), (3, 12, 4), (1, 1, 1)]
    for n, shape in enumerate(shapes):
        for fill in (0.02, 0.15, 0.6):
            seed = rng.random(shape) < fill
            if n == 0 and fill == 0.02:
                seed[...] = False
                seed[3, 4, 5] = True                      # a single seed
            got, want = mm.d2_mm(seed, spacing), mm.d2_brute(seed, spacing)
            assert got.dtype == np.float64 and np.array_equal(got.view(np.uint64), want.view(np.uint64)), (shape, fill)
    assert np.isinf(mm.d2_mm(np.zeros((3, 4, 5), bool), spacing)).all()


@pytest.mark.parametrize("spacing", mm.SPACINGS + EXTRA_SPACINGS, ids=str)
def test_restatement_is_scipys_sampled_transform(spacing):
    for shape, kind in (((19, 67, 131), "blobs"), ((1, 33, 70), "faces"), ((5, 3, 300), "corners")):
        seed = (sr.case_ref(shape, kind)["flags"] & sr.B26_T) != 0
        assert seed.any()
        got, want = mm.d2_mm(seed, spacing), ndi.distance_transform_edt(~seed, sampling=spacing) ** 2
        assert np.all(np.abs(got - want) <= 1e-12 * want), (shape, kind, float(np.abs(got - want).max()))


# ------------------------------------------------------------------------------------------------------ unit spacing
@pytest.mark.parametrize("shape", sr.SHAPES, ids=IDS)
def test_unit_spacing_reproduces_the_integer_restatements(shape):
    one = (1.0, 1.0, 1.0)
    for kind in sr.MASKS:
        ref, got = sr.case_ref(shape, kind), mm.case_ref(shape, kind, one)
        for key in ("d2T", "d2P"):
            want = np.where(ref[key] >= sr.NO_SEED, np.inf, ref[key].astype(np.float64))
            assert np.array_equal(got[key], want), (kind, key)
        words = list(got["result"])
        for k in (5, 7, 8):
            x = mm.unbits(words[k])
            assert x == int(x)
            words[k] = int(x)
        assert words == ref["result"], (kind, words, ref["result"])
        a_ref, a_got = ar.case_ref(shape, kind), mm.asd_case_ref(shape, kind, one)
        assert a_got["counts"] == a_ref["counts"]
        for key in ("sumA", "sumB"):
            assert abs(a_got[key] - a_ref[key]) <= 1e-12 * abs(a_ref[key]), (kind, key, a_got[key], a_ref[key])
        for key, w in a_ref["scores"].items():
            assert ar.same_float(a_got["scores"][key], w, 1e-12), (kind, key)


# ------------------------------------------------------------------------------------------------- a hand-worked case
def test_anisotropy_changes_the_nearest_seed():
    """seeds one voxel away along z and three voxels away along x, spacing (5, 1, 1): the nearer seed is the one 3 mm away
    (9), not the one a voxel away (5 mm: 25)"""
    seed = np.zeros((3, 1, 5), bool)
    v = (0, 0, 0)
    seed[1, 0, 0] = seed[0, 0, 3] = True
    assert mm.d2_mm(seed, (5.0, 1.0, 1.0))[v] == 9.0 == mm.d2_brute(seed, (5.0, 1.0, 1.0))[v]
    assert mm.d2_mm(seed, (1.0, 1.0, 1.0))[v] == 1.0
    assert mm._d2(seed, (5.0, 1.0, 1.0), "voxel_nearest")[v] == 25.0
    assert mm.d2_mm(seed, (1.0, 1.0, 5.0))[v] == 1.0                        # the order is that of the array's axes
    t = np.zeros((3, 4, 9), np.uint8)
    p = t.copy()
    t[1, 1, 1] = p[1, 1, 4] = p[2, 1, 1] = 1
    got = mm.scores(mm.surface(t, p, 1, (5.0, 1.0, 1.0))["result"])
    assert got["HausdorffDistance"] == 5.0                                  # from p's voxel one slice up
    assert mm.scores(mm.surface(t, p, 1, (1.0, 1.0, 1.0))["result"])["HausdorffDistance"] == 3.0


# -------------------------------------------------------------------------------------------------- planted defects
def _visible(shape, kind, spacing, defect):
    """does the defect change anything the GPU tests compare (maps and result words in every bit, sums to 1e-12)?"""
    t, p, k = sr.case(shape, kind)
    good, bad = mm.case_ref(shape, kind, spacing), mm.surface(t, p, k, spacing, defect, base=sr.case_ref(shape, kind))
    if good["result"] != bad["result"] or not np.array_equal(good["d2T"], bad["d2T"]):
        return True
    ga, ba = mm.asd_case_ref(shape, kind, spacing), mm.asd(t, p, k, spacing, defect, base=ar.case_ref(shape, kind))
    return not all(abs(ga[s] - ba[s]) <= 1e-12 * abs(ga[s]) for s in ("sumA", "sumB"))


@pytest.mark.parametrize("defect", mm.DEFECTS)
def test_gpu_inputs_can_see_each_planted_defect(defect):
    """a defect of the metric or of the sum shows on every anisotropic input; one of the ranks shows where the sorted
    distances around the 95 % rank differ, which the crafted key sets of the select guarantee"""
    shape = (19, 67, 131)
    seen = [_visible(shape, kind, spacing, defect) for spacing in ((3.0, 0.5, 0.5), (0.7, 1.3, 2.9))
            for kind in ("blobs", "faces")]
    if defect in ("hi_distinct", "rank_off"):
        hit = [name for name, keys, ranks in mm.select_cases()
               if any(mm.select_ref(keys, lo) != mm.select_ref(keys, lo, defect) for lo in ranks)]
        # (a small volume has few distinct distances, and many voxels share the one at the 95 % rank: the volumes alone
        # need not see these two, the key sets must -- the surface entry runs the same select, and reports lo and r)
        assert "two values" in hit and ("random" in hit or defect == "hi_distinct"), (defect, hit, seen)
    else:
        assert all(seen), (defect, seen)
    if defect in ("wrong_axes", "not_squared", "voxel_nearest"):            # unit spacing cannot see a metric defect
        assert not _visible(shape, "blobs", (1.0, 1.0, 1.0), defect)


def test_select_cases_are_what_they_claim():
    cases = dict((name, (keys, ranks)) for name, keys, ranks in mm.select_cases())
    assert len(cases["n=1"][0]) == 1 and len(set(cases["all equal"][0].tolist())) == 1
    assert sorted(set(cases["two values"][0].tolist())) == [7, 9]
    low = cases["lowest bit"][0]
    assert len(set(low.tolist())) == 2 and int(low.max() - low.min()) == 1
    for digit in range(4):
        keys = cases[f"digit {digit}"][0]
        diff = np.bitwise_or.reduce(keys ^ keys[0])
        assert int(diff) & ~(0xFFFF << (16 * digit)) == 0 and len(set(keys.tolist())) > 1000, digit
    keys, ranks = cases["random"]
    assert len(keys) == 70000 and {0, 69999, 95 * 69999 // 100} <= set(ranks)
    assert np.array_equal(np.sort(keys), np.sort(keys.view(np.float64)).view(np.uint64))   # bit patterns order like the doubles
    keys = np.array([7] * 5 + [9] * 3, np.uint64)
    assert [mm.select_ref(keys, lo)[1] for lo in (0, 3, 4, 6, 7)] == [7, 7, 9, 9, 9]     # the next ELEMENT
    assert mm.select_ref(keys, 0, "hi_distinct")[1] == 9


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


ENTRIES = (("hdf_surface_mm_workspace_bytes", "int64_t", 3), ("hdf_op_edt_sq_mm", "int", 10), ("hdf_op_select_u64", "int", 7),
           ("hdf_surface_distances_mm", "int", 11), ("hdf_surface_asd_mm", "int", 11))


def test_mm_entries_are_declared_exported_and_bound(lib):
    from hdf_rt import _lib
    hdr = " ".join(open(os.path.join(ROOT, "include", "hdf.h")).read().split())
    for name, ret, nargs in ENTRIES:
        assert name in _lib.EXPORTS and hasattr(lib, name) and f"{ret} {name}(" in hdr, name
        assert len(_lib._PROTOS[name][1]) == nargs, name
        decl = hdr[hdr.index(f"{ret} {name}("):]
        assert decl[:decl.index(")")].count(",") + 1 == nargs, name
    assert _lib._PROTOS["hdf_surface_mm_workspace_bytes"][0] is C.c_int64
    assert "#define HDF_SELECT_U64_WS 49408" in hdr
    spec = importlib_build()
    assert "surface_mm.hip" in spec.SOURCES


def importlib_build():
    import importlib.util
    spec = importlib.util.spec_from_file_location("hdf_build", os.path.join(ROOT, "h-denseformer_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _sp(*v):
    return (C.c_double * 3)(*v)


def test_mm_entries_refuse_a_bad_spacing_first(lib):
    """HDF_ERR_ARG (1) with a "surface:" message that names the spacing, although every other argument is bad as well: the
    spacing is a host pointer and is checked before anything else.  On a host without a device a memset or a launch would
    come back as HDF_ERR_HIP (2).  The addresses are never dereferenced."""
    buf = (C.c_uint64 * 16)()
    a = C.addressof(buf)

    def three(sp, D=0, H=0, W=0, label=0, ws_bytes=0):
        return [lib.hdf_op_edt_sq_mm(a, label, D, H, W, sp, a, a, ws_bytes, None),
                lib.hdf_surface_distances_mm(a, a, label, D, H, W, sp, a, ws_bytes, a, None),
                lib.hdf_surface_asd_mm(a, a, label, D, H, W, sp, a, ws_bytes, a, None)]

    bad = [None, _sp(0.0, 1, 1), _sp(1, -1.0, 1), _sp(1, 1, float("nan")), _sp(float("inf"), 1, 1),
           _sp(1, 1, 2.0 ** -11), _sp(1, 1025.0, 1), _sp(1, 1, 5e-324), _sp(-0.0, 1, 1)]
    for sp in bad:
        for dims in ((0, 0, 0), (8, 9, 10)):
            for rc in three(sp, *dims):
                msg = lib.hdf_last_error()
                assert rc == 1 and msg.startswith(b"surface:") and b"spacing" in msg, (sp and list(sp), rc, msg)
    assert all(buf[i] == 0 for i in range(16))


def test_mm_entries_refuse_what_the_unit_spacing_entries_refuse(lib):
    buf = (C.c_uint64 * 16)()
    a = C.addressof(buf)
    big = 1 << 40
    ok = _sp(2.0 ** -10, 1024.0, 0.7)                                       # the ends of the range are inside it

    def three(D, H, W, label, ws_bytes):
        return [lib.hdf_op_edt_sq_mm(a, label, D, H, W, ok, a, a, ws_bytes, None),
                lib.hdf_surface_distances_mm(a, a, label, D, H, W, ok, a, ws_bytes, a, None),
                lib.hdf_surface_asd_mm(a, a, label, D, H, W, ok, a, ws_bytes, a, None)]

    def refused(rcs):
        return all(rc == 1 for rc in rcs) and lib.hdf_last_error().startswith(b"surface:")

    for dims in ((0, 8, 8), (8, 0, 8), (8, 8, 0), (1025, 8, 8), (8, 1025, 8), (8, 8, 1025)):
        assert lib.hdf_surface_mm_workspace_bytes(*dims) == -1 and lib.hdf_last_error().startswith(b"surface:")
        assert refused(three(*dims, 1, big)), dims
    for label in (0, 256):
        assert refused(three(8, 8, 8, label, big)), label
    need = lib.hdf_surface_mm_workspace_bytes(8, 9, 10)
    assert need > 0 and need % 256 == 0
    assert refused(three(8, 9, 10, 1, need - 1))
    assert b"workspace" in lib.hdf_last_error()
    # null pointers with everything else in order
    assert lib.hdf_surface_distances_mm(None, a, 1, 8, 9, 10, ok, a, need, a, None) == 1
    assert lib.hdf_surface_asd_mm(a, a, 1, 8, 9, 10, ok, a, need, None, None) == 1
    assert lib.hdf_op_edt_sq_mm(a, 4, 8, 9, 10, ok, None, a, need, None) == 1
    assert lib.hdf_last_error().startswith(b"surface:")
    # the select
    for n, lo in ((0, 0), (-1, 0), (1 << 31, 0), (5, -1), (5, 5)):
        assert lib.hdf_op_select_u64(a, n, lo, a, big, a, None) == 1, (n, lo)
        assert lib.hdf_last_error().startswith(b"surface:")
    assert lib.hdf_op_select_u64(a, 5, 2, a, 49407, a, None) == 1 and b"workspace" in lib.hdf_last_error()
    assert lib.hdf_op_select_u64(None, 5, 2, a, 49408, a, None) == 1
    assert all(buf[i] == 0 for i in range(16))


def test_one_workspace_size_serves_every_entry(lib):
    """about 17 bytes a voxel (a flag byte and two fp64 maps), never below the select's own state"""
    for shape in sr.SHAPES + [(128, 128, 128), (240, 240, 155), (1024, 1024, 1024)]:
        n, v = lib.hdf_surface_mm_workspace_bytes(*shape), int(np.prod(shape))
        assert n >= 49408 + 17 * v and n % 256 == 0, shape
        assert n <= 17 * v + (1 << 17), shape


# -------------------------------------------------------------------------------------------------- the Python names
WRAPPERS = ("surface_scores", "cal_score", "multi_dice", "multi_hd", "multi_vs", "multi_jc", "asd_scores", "cal_asd",
            "multi_asd")


def test_every_wrapper_takes_spacing_and_defaults_to_none():
    import inspect

    import hdf_rt
    for name in WRAPPERS:
        par = inspect.signature(getattr(hdf_rt, name)).parameters
        assert "spacing" in par and par["spacing"].default is None, name
        assert "spacing" in getattr(hdf_rt, name).__doc__, name


def test_wrappers_with_a_spacing_fail_loudly_without_a_device(monkeypatch):
    import hdf_rt
    from hdf_rt import HdfError
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)     # (so that the test is the same where there is one)
    t, p = sr.label_maps((8, 9, 10), 1, 2)
    sp = (3.0, 0.5, 0.5)
    for name in ("multi_dice", "multi_hd", "multi_vs", "multi_jc", "multi_asd"):
        with pytest.raises(HdfError):
            getattr(hdf_rt, name)(t, p, 2, spacing=sp)
    for name in ("surface_scores", "asd_scores"):
        with pytest.raises(HdfError):
            getattr(hdf_rt, name)(t, p, [1], spacing=sp)
    for name in ("cal_score", "cal_asd"):
        with pytest.raises(HdfError):
            getattr(hdf_rt, name)(p == 1, t == 1, spacing=sp)


class _Recorder:
    """stands in for the library: records the entries called, every call succeeds and writes nothing"""

    def __init__(self):
        self.called = []

    def __getattr__(self, name):
        def fn(*_a):
            self.called.append(name)
            return 1 << 12 if name.endswith("workspace_bytes") else 0
        return fn


def test_spacing_none_never_touches_the_new_entries(monkeypatch):
    """the wrappers with the library, the device pointers and the stream replaced by stand-ins, on host tensors: None
    (given or left out) calls exactly the entries the parent commit called; a triple calls the _mm ones"""
    from hdf_rt import _volume, surface
    rec = _Recorder()
    for mod in (surface, _volume):              # (the workspace caches of surface live in _volume.WorkspaceCache)
        monkeypatch.setattr(mod, "lib", lambda: rec)
        monkeypatch.setattr(mod, "stream_ptr", lambda: 0)
    monkeypatch.setattr(surface, "_volume", lambda a, what: torch.as_tensor(np.ascontiguousarray(a)).to(torch.uint8))
    for cache in (surface._workspaces, surface._asd_workspaces, surface._mm_workspaces):
        monkeypatch.setattr(cache, "get", lambda key, default=None: None)      # every call asks the library for the size

    class _NoDevice:
        def __init__(self, *_a):
            pass

        def __enter__(self):
            return self

        def __exit__(self, *_a):
            return False

    monkeypatch.setattr(torch.cuda, "device", _NoDevice)
    monkeypatch.setattr(torch, "empty", torch.zeros)           # the rows nothing writes: all zero, not whatever was there
    t, p = sr.label_maps((4, 5, 6), 1, 2)
    for kw in ({}, {"spacing": None}):
        rec.called.clear()
        surface.multi_hd(t, p, 2, **kw), surface.multi_dice(t, p, 2, **kw), surface.cal_score(p == 1, t == 1, **kw)
        surface.surface_scores(t, p, [1, 2], **kw), surface.multi_vs(t, p, 2, **kw), surface.multi_jc(t, p, 2, **kw)
        assert set(rec.called) == {"hdf_surface_workspace_bytes", "hdf_surface_distances"}, rec.called
        rec.called.clear()
        surface.multi_asd(t, p, 2, **kw), surface.cal_asd(p == 1, t == 1, **kw), surface.asd_scores(t, p, [1], **kw)
        assert set(rec.called) == {"hdf_surface_asd_workspace_bytes", "hdf_surface_asd"}, rec.called
    rec.called.clear()
    surface.multi_hd(t, p, 2, spacing=(3, 0.5, 0.5)), surface.cal_score(p == 1, t == 1, spacing=(3, 0.5, 0.5))
    assert set(rec.called) == {"hdf_surface_mm_workspace_bytes", "hdf_surface_distances_mm"}, rec.called
    rec.called.clear()
    surface.multi_asd(t, p, 2, spacing=(3, 0.5, 0.5)), surface.cal_asd(p == 1, t == 1, spacing=(3, 0.5, 0.5))
    assert set(rec.called) == {"hdf_surface_mm_workspace_bytes", "hdf_surface_asd_mm"}, rec.called
    with pytest.raises(ValueError):
        surface.multi_hd(t, p, 2, spacing=(1.0, 1.0))
    surface.clear_workspaces()                  # the stand-in workspaces are host tensors: nothing later may find them


def test_scores_from_result_mm_reads_bit_patterns():
    from hdf_rt.surface import scores_from_result, scores_from_result_mm
    row = [10, 12, 6, 4, 5, mm.bits(6.25), 9, mm.bits(2.25), mm.bits(4.0), 7, 60, 1]
    s = scores_from_result_mm(row)
    assert s["HausdorffDistance"] == 2.5 and s["HausdorffDistance95"] == 1.5 + 0.5 * 60 / 100
    assert s["Dice"] == 12 / 22 and s == mm.scores(row)
    unit = scores_from_result([10, 12, 6, 4, 5, 9, 9, 4, 16, 7, 60, 1])
    assert unit["HausdorffDistance"] == 3.0 and unit["HausdorffDistance95"] == 2 + 2 * 60 / 100
    s = scores_from_result_mm([0, 12, 0, 0, 5, 0, 0, 0, 0, 0, 0, 0])
    assert math.isnan(s["HausdorffDistance"]) and math.isnan(s["HausdorffDistance95"]) and s["Dice"] == 0.0
