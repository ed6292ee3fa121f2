"""tests/lesion_hd_ref.py (the numpy / scipy restatement hdf_lesion_surface and hdf_rt.lesion_wise_scores(hd95=True) are
compared with) held to what it has to show without a device: the crop of a lesion's box grown by one voxel gives the twelve
words of the full volume (and the box without the margin does not), six planted defects are visible on the committed inputs
through the GPU test's own comparison, the aggregate and its empty cases, and the declarations, exports, refusals and the size
function of the library's entries, which are host arithmetic."""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest

import lesion_hd_ref as lh
from conftest import ROOT


def _kept_with_pred(name):
    _n, pred, truth, label, kw = lh.case(name)
    kw = {k: v for k, v in kw.items() if k != "min_size"}
    return [(T, P) for _j, T, touching, P in lh.lesion_masks(pred, truth, label, **kw)[5] if touching]


@pytest.mark.parametrize("spacing", [None, lh.SPACING], ids=["voxels", "mm"])
def test_the_margin_one_crop_gives_the_full_volume_words(spacing):
    lesions = tight_differs = 0
    for name in lh.CASE_NAMES:
        for T, P in _kept_with_pred(name):
            full = lh.surface_words(T, P, spacing)
            assert lh.surface_words(T, P, spacing, lh.crop_box(T | P, 1)) == full, name
            lesions += 1
            tight_differs += lh.surface_words(T, P, spacing, lh.crop_box(T | P, 0)) != full
    assert lesions >= 100 and tight_differs >= 20, (lesions, tight_differs)


def test_crop_box_clamps_and_grows():
    m = np.zeros((4, 5, 6), bool)
    m[0, 2, 5] = m[1, 3, 5] = True
    assert lh.crop_box(m, 0) == (slice(0, 2), slice(2, 4), slice(5, 6))
    assert lh.crop_box(m, 1) == (slice(0, 3), slice(1, 5), slice(4, 6))
    layout, total = lh.crop_layout([[1, 0, 1, 2, 3, 5, 5], [2, 3, 3, 0, 0, 0, 0]], (4, 5, 6))
    assert layout == [(0, lh.crop_box(m, 1)), (2 * 3 * 4 * 2, (slice(2, 4), slice(0, 2), slice(0, 2)))] and total == 48 + 16


@pytest.mark.parametrize("defect", lh.DEFECTS)
def test_planted_defect_is_caught_by_the_gpu_tests_comparison(defect):
    """every defect changes a result word or the aggregate on at least one committed input, in voxels and with the spacing"""
    for spacing in (None, lh.SPACING):
        caught = []
        for name, pred, truth, label, kw in lh.cases():
            bad = lh.mismatches(lh.lesion_hd_ref(pred, truth, label, spacing=spacing, defect=defect, **kw),
                                lh.case_ref(name, spacing))
            if bad:
                caught.append((name, bad[0]))
        assert caught, (defect, spacing)
        meant = {"tight_crop": "bar", "dilated_truth": "corner", "no_pool": "8x8x70-s2", "all_pred": "miss_and_fp",
                 "miss_scores_zero": "only_miss", "fp_unpenalised": "only_fp"}[defect]
        assert meant in [c[0] for c in caught], (defect, caught)


def test_the_comparison_sees_one_bit_and_takes_nan():
    want = lh.case_ref("full_truth")
    assert math.isnan(want["lesions"][0]["hd95"]) and want["lesions"][0]["surface"][11] == 0
    assert lh.mismatches(lh.lesion_hd_ref(*lh.case("full_truth")[1:4], **lh.case("full_truth")[4]), want) == []
    got = dict(want, lesion_hd95=np.nextafter(want["lesion_hd95"], 0.0).item())
    assert lh.mismatches(got, want) == [".lesion_hd95"]
    assert lh.mismatches(dict(want, fp=0.0), want) == [".fp"]


def test_aggregate_and_empty_cases():
    assert lh.case_ref("nothing")["lesion_hd95"] == 0.0 and lh.case_ref("nothing")["lesion_dice"] == 1.0
    r = lh.case_ref("only_fp")
    assert r["fp"] == 2 and r["lesions"] == [] and r["lesion_hd95"] == lh.PENALTY
    r = lh.case_ref("only_miss")
    assert r["fp"] == 0 and [l["surface"] for l in r["lesions"]] == [None] and r["lesion_hd95"] == lh.PENALTY
    assert r["lesions"][0]["hd"] == r["lesions"][0]["hd95"] == lh.PENALTY
    # one matched lesion, one miss, one false positive: (hd95 + 2 penalties) / 3, and another penalty goes through
    _n, pred, truth, label, kw = lh.case("miss_and_fp")
    r = lh.lesion_hd_ref(pred, truth, label, hd95_penalty=100.0, **kw)
    got = [l["hd95"] for l in r["lesions"]]
    assert r["fp"] == 1 and sorted(got)[1] == 100.0 and r["lesion_hd95"] == (got[0] + got[1] + 100.0) / 3
    # a dropped lesion neither scores nor counts; its predicted neighbour is no false positive
    r = lh.case_ref("min_size")
    assert r["dropped"] == [1] and r["fp"] == 0 and len(r["lesions"]) == 1 and r["lesion_hd95"] == r["lesions"][0]["hd95"]
    # hand-worked: a 2x2x2 truth block at the corner, the prediction a 2x3x2 block shifted by one along x
    r = lh.case_ref("corner")["lesions"][0]
    assert r["surface"][:3] == [8, 12, 4] and r["hd"] == math.sqrt(2) and r["surface"][11] == 1


def test_the_inputs_reach_what_the_kernel_can_get_wrong():
    shapes = {n: lh.case_entry(n) for n in lh.CASE_NAMES}
    lat, total = lh.crop_layout(shapes["lattice"]["lesions"], lh.LATTICE_SHAPE)
    assert len(lat) == 100 and total == 100 * 2 * 45            # more than one carve launch (64 lesions), 3x3x5 crops
    # crops of odd width whose predicted mask starts at an odd byte, in the hand-made cases
    odd = 0
    for name in lh.hand_cases():
        _n, pred, _t, _l, _kw = lh.case(name)
        for off, box in lh.crop_layout(shapes[name]["lesions"], pred.shape)[0]:
            n = [s.stop - s.start for s in box]
            odd += n[2] % 2 == 1 and (off + n[0] * n[1] * n[2]) % 2 == 1
    assert odd >= 100
    # one predicted id in two P_j, and crops that overlap
    bar = shapes["bar"]
    assert len(bar["lesions"]) == 2 and [r[:2] for r in bar["pairs"].tolist() if r[0] == 1 and r[1] > 0] == [[1, 1], [1, 2]]
    (_, a), (_, b) = lh.crop_layout(bar["lesions"], (7, 11, 19))[0]
    assert all(max(p.start, q.start) < min(p.stop, q.stop) for p, q in zip(a, b))
    # three clamped sides
    assert [s.start for s in lh.crop_layout(shapes["corner"]["lesions"], (7, 11, 19))[0][0][1]] == [0, 0, 0]
    # a crop row longer than a wave, a crop of more than one workgroup's 1024 voxels
    rows = [(s[2].stop - s[2].start, np.prod([x.stop - x.start for x in s])) for n in lh.CASE_NAMES
            for _o, s in lh.crop_layout(shapes[n]["lesions"], lh.case(n)[1].shape)[0]]
    assert max(r[0] for r in rows) > 64 and max(r[1] for r in rows) > 4 * 1024


# ------------------------------------------------------------------------------------------------ the library, on the host
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


def test_entries_are_declared_exported_and_resolve(lib):
    hdr = open(os.path.join(ROOT, "include", "hdf.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"int64_t\s+hdf_lesion_surface_workspace_bytes\s*\(\s*const\s+int32_t\s*\*\s*lesions", code)
    assert re.search(r"int\s+hdf_lesion_surface\s*\(\s*const\s+int32_t\s*\*\s*ids_pred", code)
    from hdf_rt import _lib
    for name in ("hdf_lesion_surface_workspace_bytes", "hdf_lesion_surface"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    import inspect

    import hdf_rt
    sig = inspect.signature(hdf_rt.lesion_wise_scores).parameters
    assert (sig["hd95"].default, sig["spacing"].default, sig["hd95_penalty"].default) == (False, None, 374.0)
    with pytest.raises(ValueError, match="hd95=True"):
        hdf_rt.lesion_wise_scores(np.zeros((3, 4), np.uint8), np.zeros((3, 4), np.uint8), 1, spacing=(1.0, 1.0, 1.0))
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(_lib.HdfError):
            hdf_rt.lesion_wise_scores(np.zeros((3, 4), np.uint8), np.zeros((3, 4), np.uint8), 1, hd95=True)


def _rows(*rows):
    flat = [v for r in rows for v in r]
    return (C.c_int32 * max(len(flat), 1))(*flat)


def test_size_function(lib):
    size = lib.hdf_lesion_surface_workspace_bytes
    one = _rows([1, 2, 3, 2, 3, 2, 3])                                   # a 2x2x2 box inside 8x8x8: a 4x4x4 crop
    for mm, surf in ((0, lib.hdf_surface_workspace_bytes), (1, lib.hdf_surface_mm_workspace_bytes)):
        assert size(one, 1, 8, 8, 8, mm) == 256 + surf(4, 4, 4)          # 128 bytes of crops, the scratch on a 256-byte boundary
        assert size(one, 0, 8, 8, 8, mm) == 0 and size(None, 0, 8, 8, 8, mm) == 0
        # clamped on every side: the crop is the volume
        assert size(_rows([7, 0, 1, 0, 2, 0, 3]), 1, 2, 3, 4, mm) == 256 + surf(2, 3, 4)
        # two lesions: the crops add up, the scratch is the larger one's
        two = _rows([1, 2, 3, 2, 3, 2, 3], [2, 0, 5, 0, 0, 0, 0])        # 4x4x4 and 7x2x2
        assert size(two, 2, 8, 8, 8, mm) == 256 + max(surf(4, 4, 4), surf(7, 2, 2))
        # monotone in the boxes: growing any side of any box never shrinks the size
        rng = np.random.default_rng(3)
        for _ in range(200):
            dims = [int(v) for v in rng.integers(1, 40, 3)]
            box = []
            for d in dims:
                lo = int(rng.integers(0, d))
                box += [lo, int(rng.integers(lo, d))]
            base = size(_rows([1] + box), 1, *dims, mm)
            assert base > 0
            for k in range(6):
                grown = list(box)
                grown[k] += -1 if k % 2 == 0 else 1
                if grown[k] < 0 or grown[k] >= dims[k // 2]:
                    continue
                assert size(_rows([1] + grown), 1, *dims, mm) >= base, (dims, box, k)
            assert size(_rows([1] + box, [2] + box), 2, *dims, mm) >= base

    def refused(n, what):
        assert n == -1 and lib.hdf_last_error().startswith(b"surface:"), (what, n, lib.hdf_last_error())

    for dims in [(0, 8, 8), (8, 1025, 8), (8, 8, -1)]:
        refused(size(one, 1, *dims, 0), dims)
    refused(size(one, -1, 8, 8, 8, 0), "L < 0")
    refused(size(None, 1, 8, 8, 8, 0), "no rows")
    refused(size(one, 1, 8, 8, 8, 2), "mm = 2")
    for row in BAD_ROWS:
        refused(size(_rows(row), 1, 8, 8, 8, 0), row)
        refused(size(_rows([1, 2, 3, 2, 3, 2, 3], row), 2, 8, 8, 8, 1), row)


# rows an 8x8x8 volume refuses: j < 1, min > max, a box that leaves the volume on either side of any axis
BAD_ROWS = [[0, 2, 3, 2, 3, 2, 3], [-4, 2, 3, 2, 3, 2, 3], [1, 3, 2, 2, 3, 2, 3], [1, 2, 3, 5, 4, 2, 3], [1, 2, 3, 2, 3, 7, 6],
            [1, -1, 3, 2, 3, 2, 3], [1, 2, 8, 2, 3, 2, 3], [1, 2, 3, -2, 3, 2, 3], [1, 2, 3, 2, 9, 2, 3], [1, 2, 3, 2, 3, -1, 3],
            [1, 2, 3, 2, 3, 2, 8], [1, 8, 8, 2, 3, 2, 3]]


def test_entry_refuses_before_launch(lib):
    """HDF_ERR_ARG (1) with a "surface:" message.  This host has no device: anything that got as far as a launch would come
    back as HDF_ERR_HIP (2).  Every call here is a refusal, so nothing can launch and the device addresses are never
    dereferenced; the accepted forms run on device memory in tests/test_gpu_lesion_hd.py."""
    rows = _rows([1, 2, 3, 2, 3, 2, 3], [2, 0, 5, 0, 0, 0, 0])
    need = lib.hdf_lesion_surface_workspace_bytes(rows, 2, 8, 8, 8, 1)
    assert need >= lib.hdf_lesion_surface_workspace_bytes(rows, 2, 8, 8, 8, 0) > 0
    buf = (C.c_uint8 * (3 * 8192 + need))()
    a = (C.addressof(buf) + 63) // 64 * 64
    ip, it, mask, pairs, res, ws = a, a + 2048, a + 4096, a + 4608, a + 8192, a + 8192 + 256       # 8x8x8: 2048, 2048, 512
    sp = (C.c_double * 3)(2.5, 0.8, 1.1)

    def call(ip=ip, it=it, mask=mask, dims=(8, 8, 8), pairs=pairs, n_pairs=4, rows=rows, L=2, sp=None, ws=ws, ws_bytes=need,
             res=res):
        return lib.hdf_lesion_surface(ip, it, mask, *dims, pairs, n_pairs, rows, L, sp, ws, ws_bytes, res, None)

    def refused(rc, what):
        assert rc == 1 and lib.hdf_last_error().startswith(b"surface:"), (what, rc, lib.hdf_last_error())

    for dims in [(0, 8, 8), (8, 1025, 8), (8, 8, -1), (1025, 1, 1)]:
        refused(call(dims=dims, ws_bytes=1 << 40), "dimension %s" % (dims,))
    refused(call(L=-1), "L < 0")
    refused(call(n_pairs=-1), "n_pairs < 0")
    for name in ("ip", "it", "mask", "pairs", "rows", "res", "ws"):
        refused(call(**{name: None}), "null " + name)
    for row in BAD_ROWS:
        refused(call(rows=_rows(row), L=1), row)
        refused(call(rows=_rows([1, 2, 3, 2, 3, 2, 3], row), sp=sp), row)
    for bad in [(0.0, 1.0, 1.0), (1.0, float("nan"), 1.0), (1.0, 1.0, 4096.0)]:
        refused(call(sp=(C.c_double * 3)(*bad)), "spacing %s" % (bad,))
    refused(call(ws_bytes=lib.hdf_lesion_surface_workspace_bytes(rows, 2, 8, 8, 8, 0) - 1), "short workspace")
    refused(call(sp=sp, ws_bytes=need - 1), "short workspace with a spacing")
    refused(call(ws=ws + 4), "workspace not aligned")
    need0 = lib.hdf_lesion_surface_workspace_bytes(rows, 2, 8, 8, 8, 0)          # (what a call without a spacing uses)
    refused(call(res=ws + need0 - 8), "results overlaps the workspace from above")
    refused(call(sp=sp, res=ws + need - 8), "results overlaps the workspace from above, with a spacing")
    refused(call(res=ws - 2 * 96 + 8), "results overlaps the workspace from below")
    refused(call(res=ip + 2040), "results overlaps ids_pred")
    refused(call(res=mask + 8), "results overlaps the mask")
    refused(call(res=pairs + 4 * 32 - 8), "results overlaps pairs")
    refused(call(ws=it + 2040), "workspace overlaps ids_truth")
    # and the accepted corner of the contract: no lesions is no work, whatever the workspace
    assert call(L=0, ws=None, ws_bytes=0, res=None, rows=None) == 0


# ------------------------------------------------------------------------------------------------ the code object
sys.path.insert(0, os.path.join(ROOT, "tools"))
import codeobj  # noqa: E402


@pytest.mark.skipif(not os.path.exists(codeobj.LIB), reason="libhdf_hip.so not built")
def test_the_carve_kernel_uses_no_scratch():
    ks = codeobj.kernels()
    names = [n for n in ks if "lesion_carve_kernel" in n]
    assert len(names) == 1
    k = ks[names[0]]
    assert not k.get("private_segment_fixed_size", 0) and not k.get("vgpr_spill_count", 0), k
    assert k.get("group_segment_fixed_size", 0) == 0 and k["max_flat_workgroup_size"] == 256
