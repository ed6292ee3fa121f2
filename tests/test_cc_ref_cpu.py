"""tests/cc_ref.py (the scipy restatement the GPU kernels are compared with) held to a flood fill written independently:
an explicit neighbour list, a stack, ids handed out in raster order; table and filter by plain loops.  Volumes up to
9x10x11, all three connectivities, one value and three.  Then six defects planted in copies of the flood fill, each of
which the comparison of the GPU test (cc_ref.mismatches, over cc_ref's masks) must catch, and the refusals of the
library's entries, which need no device."""
import ctypes as C
import os

import numpy as np
import pytest
from scipy import ndimage as ndi

import cc_ref as cr
from conftest import ROOT

DEFECTS = ("conn18_for_26", "row_wrap", "merge_values", "order_by_size", "tie_to_larger_id", "min_size_strict")
SMALL = [(1, 1, 1), (1, 7, 9), (3, 4, 5), (2, 2, 2), (9, 10, 11), (7, 9, 11), (5, 1, 6)]


def neighbours(connectivity):
    """the offsets written out: faces, then edges, then corners"""
    faces = [(-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)]
    edges = [(a, b, 0) for a in (-1, 1) for b in (-1, 1)] + [(a, 0, b) for a in (-1, 1) for b in (-1, 1)] + \
            [(0, a, b) for a in (-1, 1) for b in (-1, 1)]
    corners = [(a, b, c) for a in (-1, 1) for b in (-1, 1) for c in (-1, 1)]
    return {6: faces, 18: faces + edges, 26: faces + edges + corners}[connectivity]


def brute(vol, connectivity, label, score, min_sizes, defect=None):
    """a dict shaped like cc_ref.full's, by flood fill"""
    assert defect is None or defect in DEFECTS
    D, H, W = vol.shape
    offs = neighbours(18 if defect == "conn18_for_26" and connectivity == 26 else connectivity)
    flat = vol.ravel()
    V = flat.size
    ids = np.zeros(V, np.int64)
    comps = []                                          # voxel lists, in raster order of their first voxel
    for s in range(V):
        if ids[s] or flat[s] == 0 or (label and flat[s] != label):
            continue
        comps.append([])
        ids[s] = len(comps)
        stack = [s]
        while stack:
            v = stack.pop()
            comps[-1].append(v)
            z, y, x = v // (H * W), v // W % H, v % W
            for dz, dy, dx in offs:
                n = v + (dz * H + dy) * W + dx
                if defect == "row_wrap":                # x by the linear index alone: x = W - 1 joins x = 0 of the next row
                    ok = 0 <= z + dz < D and 0 <= y + dy < H and 0 <= n < V
                else:
                    ok = 0 <= z + dz < D and 0 <= y + dy < H and 0 <= x + dx < W
                if not ok or ids[n] or flat[n] == 0 or (label and flat[n] != label):
                    continue
                if flat[n] != flat[v] and defect != "merge_values":
                    continue
                ids[n] = len(comps)
                stack.append(n)
    if defect == "order_by_size":
        order = sorted(range(len(comps)), key=lambda i: (-len(comps[i]), min(comps[i])))
        comps = [comps[i] for i in order]
        for i, c in enumerate(comps, 1):
            ids[c] = i
    n = len(comps)
    table = np.zeros((n, 9), np.int64)
    smax = np.zeros(n, np.float32)
    sflat = score.ravel()
    for i, c in enumerate(comps):
        c = np.asarray(c)
        z, y, x = c // (H * W), c // W % H, c % W
        table[i] = [len(c), flat[c.min()], c.min(), z.min(), z.max(), y.min(), y.max(), x.min(), x.max()]
        smax[i] = sflat[c].max()
    out = dict(ids=ids.reshape(vol.shape), result=[n, int((ids > 0).sum())], table=table, score_max=smax, filters={})
    winner = {}                                         # value -> the largest component, the first of equals
    for i, c in enumerate(comps):
        u = int(table[i, 1])
        if u not in winner:
            winner[u] = i
        elif len(c) > len(comps[winner[u]]) or (defect == "tie_to_larger_id" and len(c) == len(comps[winner[u]])):
            winner[u] = i
    for ms in min_sizes:
        for kl in (0, 1):
            keep = []
            for i, c in enumerate(comps):
                k = len(c) > ms if defect == "min_size_strict" else len(c) >= ms
                keep.append(k and (not kl or winner[int(table[i, 1])] == i))
            o = np.zeros(V, np.uint8)
            for i, c in enumerate(comps):
                if keep[i]:
                    o[c] = flat[c]
            out["filters"][(ms, kl)] = (o.reshape(vol.shape), [sum(keep), int((o > 0).sum())])
    return out


def _volumes(shape):
    rng = np.random.default_rng(sum(shape))
    for dens in (0.2, 0.5, 0.8):
        fg = rng.random(shape) < dens
        yield "one value %.1f" % dens, (fg * 2).astype(np.uint8)
        yield "three values %.1f" % dens, (fg * rng.integers(1, 4, shape)).astype(np.uint8)


@pytest.mark.parametrize("shape", SMALL, ids=lambda s: "x".join(map(str, s)))
def test_restatement_equals_flood_fill_in_every_element(shape):
    score = cr.score_of(shape)
    for name, vol in _volumes(shape):
        for c in cr.CONNECTIVITIES:
            for lab in (0, 2):
                want = cr.full(vol, c, lab, score)
                got = brute(vol, c, lab, score, want["min_sizes"])
                assert cr.mismatches(got, want) == [], (name, c, lab)
                assert cr.mismatches(want, got) == []


def test_the_masks_of_the_gpu_test_on_small_volumes():
    """every mask kind of cc_ref on two small shapes: restatement against flood fill"""
    for shape in [(5, 6, 7), (1, 6, 9), (4, 5, 8)]:
        score = cr.score_of(shape)
        for kind in cr.MASKS:
            vol = cr.case.__wrapped__(shape, kind)
            for c in cr.CONNECTIVITIES:
                for lab in (0, 2):
                    want = cr.full(vol, c, lab, score)
                    assert cr.mismatches(brute(vol, c, lab, score, want["min_sizes"]), want) == [], (shape, kind, c, lab)


def test_known_counts():
    shape = (4, 6, 8)
    chk = cr.case.__wrapped__(shape, "checker")
    assert cr.label(chk, 6)[1] == 4 * 6 * 8 // 2 and cr.label(chk, 18)[1] == 1 and cr.label(chk, 26)[1] == 1
    ser = cr.case.__wrapped__((5, 7, 9), "serpentine")
    for c in cr.CONNECTIVITIES:
        assert cr.label(ser, c)[1] == 1
    # a pure path under 6-connectivity: every voxel but the two ends has exactly two face neighbours
    nb = ndi.convolve((ser > 0).astype(int), cr.STRUCTURE[6].astype(int), mode="constant") - 1
    assert sorted(np.bincount(nb[ser > 0]).tolist()) == [0, 2, int((ser > 0).sum()) - 2]
    comb = cr.case.__wrapped__((5, 7, 9), "comb")
    assert cr.label(comb, 26)[1] == 1 and cr.label(comb[:, :-1], 26)[1] == 3 * 5
    wrap = cr.case.__wrapped__((5, 7, 9), "wrap")
    assert cr.label(wrap, 26)[1] == int((wrap > 0).sum())          # nothing joins across a row or a plane end
    ec = cr.case.__wrapped__((5, 7, 45), "edge_corner")
    assert cr.label(ec, 6)[1] > cr.label(ec, 18)[1] > cr.label(ec, 26)[1]
    planes = cr.case.__wrapped__((5, 7, 9), "planes2")
    assert cr.label(planes, 26)[1] == 5 and cr.label(planes, 26, 2)[1] == 3
    tie = cr.case.__wrapped__((5, 7, 45), "tie")
    t = cr.full(tie, 26, 0)
    assert t["table"][:, 0].tolist() == [2, 2, 1, 1, 2, 2] and t["table"][:, 1].tolist() == [2, 2, 2, 3, 3, 3]
    kept = t["filters"][(0, 1)][0]
    assert np.unique(cr.label(kept, 26)[0][kept > 0]).tolist() == [1, 2]
    assert sorted(np.flatnonzero(kept.ravel()).tolist()) == [0, 1, 18, 19]


def test_depth_one_is_the_two_dimensional_case():
    rng = np.random.default_rng(3)
    for shape in [(7, 9), (10, 11)]:
        for dens in (0.3, 0.6):
            m = rng.random(shape) < dens
            four, eight = ndi.generate_binary_structure(2, 1), np.ones((3, 3), bool)
            for c, s in ((6, four), (18, eight), (26, eight)):
                want, n = ndi.label(m, s)
                got, k = cr.label((m[None] * 2).astype(np.uint8), c)
                assert k == n and np.array_equal(got[0], want)


@pytest.mark.parametrize("defect", DEFECTS)
def test_planted_defect_is_caught_by_the_gpu_tests_comparison(defect):
    """on small versions of the GPU test's own masks: at least one (mask, connectivity, label) must show the defect, and
    the clean flood fill must show nothing on the same inputs"""
    caught = []
    for shape in [(2, 3, 30), (1, 6, 9)]:
        score = cr.score_of(shape)
        for kind in cr.MASKS:
            vol = cr.case.__wrapped__(shape, kind)
            for c in cr.CONNECTIVITIES:
                for lab in (0, 2):
                    want = cr.full(vol, c, lab, score)
                    bad = cr.mismatches(brute(vol, c, lab, score, want["min_sizes"], defect), want)
                    if bad:
                        caught.append((shape, kind, c, lab, bad[0]))
    assert caught, defect
    # the masks meant for the defect are among those that catch it
    meant = {"conn18_for_26": "edge_corner", "row_wrap": "wrap", "merge_values": "planes2", "order_by_size": "tie",
             "tie_to_larger_id": "tie", "min_size_strict": "tie"}[defect]
    assert any(k[1] == meant for k in caught), (defect, sorted({k[1] for k in caught}))


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


def test_workspace_size_refuses_bad_dimensions(lib):
    assert lib.hdf_cc_workspace_bytes(0, 4, 4) == -1 and lib.hdf_cc_workspace_bytes(4, 1025, 4) == -1
    assert lib.hdf_cc_workspace_bytes(4, 4, -1) == -1
    assert lib.hdf_last_error().startswith(b"components:")
    for shape in [(1, 1, 1), (19, 67, 131), (448, 512, 512), (1024, 1024, 1024)]:
        n = lib.hdf_cc_workspace_bytes(*shape)
        v = shape[0] * shape[1] * shape[2]
        assert 5 * v <= n <= 5 * v + v // 64 + 4096, (shape, n)


def test_entries_refuse_before_launch(lib):
    """HDF_ERR_ARG (1) with a "components:" message.  This host has no device: anything that got as far as a launch or a
    memset would come back as HDF_ERR_HIP (2).  The addresses are never dereferenced."""
    buf = (C.c_uint8 * 8192)()
    a = C.addressof(buf)
    vol, ids, res, ws, out, tab = a, a + 1024, a + 3072, a + 4096, a + 5120, a + 6144      # 4x4x4: 64 and 256 bytes
    need = lib.hdf_cc_workspace_bytes(4, 4, 4)

    def refused(rc, what):
        assert rc == 1 and lib.hdf_last_error().startswith(b"components:"), (what, rc, lib.hdf_last_error())

    refused(lib.hdf_cc_label(vol, 0, 8, 4, 4, 4, ids, res, ws, need, None), "connectivity 8")
    refused(lib.hdf_cc_label(vol, 0, 26, 4, 4, 4, ids, res, ws, need - 1, None), "short workspace")
    refused(lib.hdf_cc_label(vol, 256, 26, 4, 4, 4, ids, res, ws, need, None), "label 256")
    refused(lib.hdf_cc_label(vol, -1, 26, 4, 4, 4, ids, res, ws, need, None), "label -1")
    refused(lib.hdf_cc_label(vol, 0, 26, 4, 0, 4, ids, res, ws, need, None), "dimension 0")
    refused(lib.hdf_cc_label(vol, 0, 26, 4, 4, 1025, ids, res, ws, 1 << 40, None), "dimension 1025")
    refused(lib.hdf_cc_label(vol, 0, 26, 4, 4, 4, None, res, ws, need, None), "null ids")
    refused(lib.hdf_cc_label(vol, 0, 26, 4, 4, 4, ids, None, ws, need, None), "null result")
    refused(lib.hdf_cc_label(vol, 0, 26, 4, 4, 4, vol + 60, res, ws, need, None), "ids overlaps volume")
    refused(lib.hdf_cc_label(vol + 255, 0, 26, 4, 4, 4, vol, res, ws, need, None), "ids overlaps volume from below")
    refused(lib.hdf_cc_table(vol, ids, None, 4, 4, 4, 0, tab, None, None), "capacity 0")
    refused(lib.hdf_cc_table(vol, ids, vol, 4, 4, 4, 8, tab, None, None), "score without score_max")
    refused(lib.hdf_cc_table(vol, None, None, 4, 4, 4, 8, tab, None, None), "null ids")
    refused(lib.hdf_cc_filter(vol, ids, 4, 4, 4, -1, 0, out, res, ws, need, None), "min_size -1")
    refused(lib.hdf_cc_filter(vol, ids, 4, 4, 4, 0, 0, out, res, ws, need - 1, None), "short workspace")
    refused(lib.hdf_cc_filter(vol, ids, 4, 4, 4, 0, 0, None, res, ws, need, None), "null out")
    refused(lib.hdf_cc_filter(vol, ids, 4, 4, 4, 0, 0, ids + 8, res, ws, need, None), "out overlaps ids")


def test_python_surface_is_exported_and_has_no_cpu_path():
    import hdf_rt
    from hdf_rt import _lib
    for name in ("connected_components", "component_table", "component_stats", "keep_largest_component",
                 "remove_small_components"):
        assert name in dir(hdf_rt) and callable(getattr(hdf_rt, name))
    for name in ("hdf_cc_workspace_bytes", "hdf_cc_label", "hdf_cc_table", "hdf_cc_filter"):
        assert name in _lib.EXPORTS
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(_lib.HdfError):
            hdf_rt.connected_components(np.zeros((2, 3, 4), np.uint8))
        with pytest.raises(_lib.HdfError):
            hdf_rt.keep_largest_component(torch.zeros((3, 4), dtype=torch.bool))
