"""tests/morph_ref.py, the numpy restatement that test_gpu_morphology.py compares the kernels with, held to live scipy; the
planted defects; the new entries of the C ABI.  No GPU.

(a) morph_ref.morph / fill_holes against scipy.ndimage.binary_dilation / _erosion / _opening / _closing / _fill_holes in
    every byte: connectivity 6 / 18 / 26, border_value 0 / 1, iterations 1 / 2 / 3, every shape and mask of the GPU test;
    the depth-1 shapes against scipy's 2-D calls; MAP mode against a three-line statement of its rule.
(b) eight ways the kernels could be wrong, planted in the restatement: morph_ref.mismatches must report each on at least
    one case of the GPU test's own case list.
(c) the prototypes stand in include/hdf.h, in hdf_rt._lib.EXPORTS and in the built library; the refusals on the host."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest
from scipy import ndimage as ndi

import morph_ref as mr
from conftest import ROOT

SCIPY_OP = {mr.DILATE: ndi.binary_dilation, mr.ERODE: ndi.binary_erosion, mr.OPEN: ndi.binary_opening,
            mr.CLOSE: ndi.binary_closing}
IDS = ["%s-%s" % ("x".join(map(str, s)), k) for s, k in mr.CASES]


def _scipy_view(mask, connectivity):
    """(the array and the structuring element scipy is given): 2-D for a depth-1 volume"""
    c = mr.C_OF[connectivity]
    if mask.shape[0] == 1:
        return mask[0], ndi.generate_binary_structure(2, min(c, 2))
    return mask, ndi.generate_binary_structure(3, c)


# ------------------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize("shape,kind", mr.CASES, ids=IDS)
def test_restatement_equals_scipy_in_every_byte(shape, kind):
    vol = mr.case(shape, kind)
    for label in (0, 2):
        mask = mr.in_mask(vol, label)
        for conn in mr.CONNECTIVITIES:
            arr, structure = _scipy_view(mask, conn)
            for op, bv, n in itertools.product(mr.OPS, (0, 1), (1, 2, 3)):
                want = SCIPY_OP[op](arr, structure, iterations=n, border_value=bv).reshape(shape)
                out, res = mr.morph(vol, label, op, conn, n, bv, mr.MASK)
                assert out.dtype == np.uint8 and np.array_equal(out, want.astype(np.uint8)), (label, conn, op, bv, n)
                assert res == [int(want.sum()), int((want ^ mask).sum())]
            want = ndi.binary_fill_holes(arr, structure).reshape(shape)
            out, res = mr.fill_holes(vol, label, conn, mr.MASK)
            assert np.array_equal(out, want.astype(np.uint8)), (label, conn, "fill")
            assert res == [int(want.sum()), int((want ^ mask).sum())]


@pytest.mark.parametrize("shape,kind", [(s, k) for s, k in mr.CASES if s in ((40, 48, 56), (4, 5, 33), (1, 37, 70))],
                         ids=lambda v: str(v).replace(" ", ""))
def test_map_mode_is_its_three_line_rule(shape, kind):
    vol = mr.case(shape, kind)
    label = 2
    old = vol == label
    calls = [(mr.morph(vol, label, op, 18, 2, 0, mr.MASK), mr.morph(vol, label, op, 18, 2, 0, mr.MAP)) for op in mr.OPS]
    calls.append((mr.fill_holes(vol, label, 6, mr.MASK), mr.fill_holes(vol, label, 6, mr.MAP)))
    for (mask_out, mask_res), (map_out, map_res) in calls:
        new = mask_out.astype(bool)
        want = vol.copy()
        want[old & ~new] = 0
        want[new & ~old & (vol == 0)] = label
        assert np.array_equal(map_out, want) and map_res == mask_res
        other = (vol != 0) & (vol != label)
        assert np.array_equal(map_out[other], vol[other])


def test_the_inputs_are_what_their_names_say():
    """the gap of box_gap is closed for a 6-connected background and open for 18 / 26; the hole of hole_face is never
    filled; the object inside nested's hole survives the fill; contact holds two classes that touch"""
    for shape in ((19, 67, 131), (40, 48, 56), (4, 5, 33)):
        box, gap = mr.case(shape, "box"), mr.case(shape, "box_gap")
        assert mr.fill_holes(box, 0, 6, mr.MASK)[1][1] > 0
        assert mr.fill_holes(gap, 0, 6, mr.MASK)[1][1] > 0
        assert mr.fill_holes(gap, 0, 18, mr.MASK)[1][1] == 0 and mr.fill_holes(gap, 0, 26, mr.MASK)[1][1] == 0
        assert mr.fill_holes(mr.case(shape, "hole_face"), 0, 6, mr.MASK)[1][1] == 0
    nested = mr.case((19, 67, 131), "nested")
    assert ndi.label(nested)[1] >= 2 and mr.fill_holes(nested, 0, 6, mr.MASK)[1][1] > 0
    contact = mr.case((40, 48, 56), "contact")
    assert set(np.unique(contact)) == {0, 1, 2} and ndi.label(contact != 0)[1] == 1
    assert len(set(np.unique(mr.case((40, 48, 56), "rand50")))) == 4


# ------------------------------------------------------------------------------------------------------ (b)
def _caught(defect):
    """the first case of the GPU test's list on which the comparison notices the defect"""
    fill = defect == "face_hole_filled"
    for index, (shape, kind) in enumerate(mr.CASES):
        if defect == "flat_z_border" and shape[0] != 1:
            continue
        vol = mr.case(shape, kind)
        if fill:
            for conn, mode, label in mr.FILL_PARAMS:
                if mr.mismatches(mr.fill_holes(vol, label, conn, mode, defect), mr.fill_holes(vol, label, conn, mode)):
                    return shape, kind, conn, mode, label
        else:
            for conn, op, bv, n, mode, label in mr.morph_params(index):
                if n > 3 and vol.size > 20000:
                    continue                                  # (the short runs show every defect; keeps this quick)
                bad = mr.morph(vol, label, op, conn, n, bv, mode, defect)
                if mr.mismatches(bad, mr.morph(vol, label, op, conn, n, bv, mode)):
                    return shape, kind, conn, op, bv, n, mode, label
    return None


@pytest.mark.parametrize("defect", mr.DEFECTS)
def test_planted_defect_is_reported(defect):
    assert len(mr.DEFECTS) >= 7
    assert _caught(defect) is not None, defect


def test_the_case_list_runs_every_combination():
    seen = set()
    for index in range(len(mr.CASES)):
        seen.update(mr.morph_params(index))
    assert len(seen) == 3 * 4 * 2 * 4 * 3
    assert {p[3] for p in seen} == {1, 2, 3, 17}
    for index in range(len(mr.CASES)):
        assert {p[0] for p in mr.morph_params(index)} == {6, 18, 26}
    for k in range(len(mr.SHAPES)):                               # every shape runs every combination
        per_shape = set()
        for index in range(k * len(mr.MASKS), (k + 1) * len(mr.MASKS)):
            assert mr.CASES[index][0] == mr.SHAPES[k]
            per_shape.update(mr.morph_params(index))
        assert len(per_shape) == 288


def test_mismatches_is_exact():
    vol = mr.case((4, 5, 33), "rand50")
    good = mr.morph(vol, 0, mr.DILATE, 6, 1, 0, mr.MASK)
    assert mr.mismatches(good, good) == []
    flipped = good[0].copy()
    flipped[3, 4, 32] ^= 1
    assert mr.mismatches((flipped, good[1]), good) == ["out"]
    assert mr.mismatches((good[0], [good[1][0], good[1][1] + 1]), good) == ["result"]


# ------------------------------------------------------------------------------------------------------ (c)
NEW = ("hdf_morph_workspace_bytes", "hdf_morph", "hdf_fill_holes_workspace_bytes", "hdf_fill_holes")


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


def test_the_entries_are_declared_bound_and_exported(lib):
    from hdf_rt import _lib
    hdr = open(os.path.join(ROOT, "include", "hdf.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), name + " has no prototype in include/hdf.h"
        assert name in _lib.EXPORTS, name + " is not in hdf_rt._lib.EXPORTS"
        assert hasattr(lib, name), name + " is not exported by the library"
    consts = dict(re.findall(r"#define\s+(HDF_MORPH_[A-Z]+)\s+(\d+)", code))
    assert {k: int(v) for k, v in consts.items()} == {
        "HDF_MORPH_DILATE": mr.DILATE, "HDF_MORPH_ERODE": mr.ERODE, "HDF_MORPH_OPEN": mr.OPEN, "HDF_MORPH_CLOSE": mr.CLOSE,
        "HDF_MORPH_MASK": mr.MASK, "HDF_MORPH_MAP": mr.MAP}


def test_workspace_sizes(lib):
    """two packed buffers of ceil(W / 32) words a row, each rounded up to 256 bytes; fill holes: more than the complement,
    the ids, the flags and the labelling's own workspace together"""
    for D, H, W in mr.SHAPES + [(448, 512, 512)]:
        one = (D * H * ((W + 31) // 32) * 4 + 255) // 256 * 256
        assert lib.hdf_morph_workspace_bytes(D, H, W) == 2 * one
        V = D * H * W
        n = lib.hdf_fill_holes_workspace_bytes(D, H, W)
        assert V + 4 * V + V + 1 + lib.hdf_cc_workspace_bytes(D, H, W) <= n <= 12 * V + 8192
    for bad in ((0, 4, 4), (4, 1025, 4), (4, 4, -1)):
        assert lib.hdf_morph_workspace_bytes(*bad) == -1 and lib.hdf_last_error().startswith(b"morphology:")
        assert lib.hdf_fill_holes_workspace_bytes(*bad) == -1 and lib.hdf_last_error().startswith(b"morphology:")


def test_refusals_on_the_host(lib):
    """every refusal returns HDF_ERR_ARG (1) with a "morphology:" message before anything is launched: this host has no
    device, where a launch or a memset would come back as HDF_ERR_HIP (2).  The addresses are never dereferenced."""
    shape = (4, 5, 6)
    need, fill_need = lib.hdf_morph_workspace_bytes(*shape), lib.hdf_fill_holes_workspace_bytes(*shape)
    assert 0 < need < fill_need
    arena = (C.c_uint8 * (fill_need + 4096))()
    base = (C.addressof(arena) + 255) // 256 * 256
    vol, out, res, ws = base, base + 512, base + 1024, base + 2048
    listed = mr.refusals(vol, out, res, ws, need, fill_need, shape)
    assert len(listed) >= 40
    for what, entry, args in listed:
        rc = getattr(lib, entry)(*args)
        assert rc == 1 and lib.hdf_last_error().startswith(b"morphology:"), (what, entry, rc, lib.hdf_last_error())
    # 2^31 voxels cannot be reached with dimensions of at most 1024 (2^30): the check stands behind the cap
    assert lib.hdf_morph_workspace_bytes(1024, 1024, 1024) > 0
