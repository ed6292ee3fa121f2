"""tests/lesion_ref.py (the numpy / scipy restatement the GPU kernels and hdf_rt.lesions are compared with) held to code
written independently: pairs_ref to a triple Python loop on small volumes, the two protocol restatements to hand-worked
cases.  Then seven defects planted in copies of the loop, each of which the comparison of the GPU test
(lesion_ref.mismatches) must catch; the declarations, exports and refusals of the library's entries, which need no
device; and what hipcc made of the new kernels (no scratch)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import lesion_ref as lr
from conftest import ROOT

DEFECTS = ("unsorted", "a0_dropped", "m_over_b", "overflow_at_capacity", "run_across_row", "negative_counted",
           "m_without_mask_test")
SMALL = [(1, 1, 1), (1, 1, 65), (1, 3, 70), (2, 5, 37), (3, 4, 5), (2, 7, 9)]


def brute(ids_a, ids_b, mask, flags, capacity, defect=None):
    """(pairs, result) by a triple loop over a dict; the voxels walked as the kernel's waves walk them (64 consecutive
    voxels a wave) where a defect needs that"""
    assert defect is None or defect in DEFECTS
    D, H, W = ids_a.shape
    table, order = {}, []
    b_under = {}
    prev_key, doubled = None, False
    for z in range(D):
        for y in range(H):
            for x in range(W):
                v = (z * H + y) * W + x
                a, b = int(ids_a[z, y, x]), int(ids_b[z, y, x])
                if defect == "negative_counted":
                    a, b = abs(a), abs(b)
                a, b = max(a, 0), max(b, 0)
                under = mask is not None and mask[z, y, x] != 0
                if defect == "m_without_mask_test":
                    under = mask is not None and mask[z, y, x] == 255
                counted = (a > 0 and b > 0) or (flags & lr.A0 and a == 0 and b > 0 and defect != "a0_dropped") or \
                          (flags & lr.B0 and a > 0 and b == 0)
                key = (a, b) if counted else None
                if under and b > 0:
                    b_under[b] = b_under.get(b, 0) + 1
                # a run that does not stop at a row start while the row start opens one as well: its voxels on the new row,
                # up to the end of the run or of the wave, are counted twice
                if v % 64 == 0 or key is None or key != prev_key:
                    doubled = False
                elif x == 0:
                    doubled = defect == "run_across_row"
                prev_key = key
                if key is None:
                    continue
                if key not in table:
                    table[key] = [0, 0]
                    order.append(key)
                table[key][0] += 2 if doubled else 1
                table[key][1] += (2 if doubled else 1) * int(under)
    keys = order if defect == "unsorted" else sorted(table)
    pairs = np.zeros((capacity, 4), np.int64)
    over = len(keys) >= capacity if defect == "overflow_at_capacity" else len(keys) > capacity
    if over:
        return pairs, [0, 0, 0, 1]
    for r, k in enumerate(keys):
        m = b_under.get(k[1], 0) if defect == "m_over_b" and k[1] > 0 else table[k][1]
        pairs[r] = [k[0], k[1], table[k][0], m]
    return pairs, [len(keys), int(pairs[:, 2].sum()), int(pairs[:, 3].sum()), 0]


def _inputs(shape):
    """(kind, mask kind, ids_a, ids_b, mask) of the GPU test's own maps and masks on one shape"""
    for kind in lr.MAPS:
        a, b = lr.id_maps(shape, kind)
        for mk in lr.MASKS:
            yield kind, mk, a, b, lr.mask_of(shape, mk)


@pytest.mark.parametrize("shape", SMALL, ids=lambda s: "x".join(map(str, s)))
def test_pairs_restatement_equals_the_triple_loop(shape):
    for kind, mk, a, b, mask in _inputs(shape):
        for flags in lr.FLAGS:
            P = lr.pairs_ref(a, b, mask, flags, 1 << 16)[1][0]
            for cap in sorted({1, max(P - 1, 1), max(P, 1), P + 3}):
                want = lr.pairs_ref(a, b, mask, flags, cap)
                got = brute(a, b, mask, flags, cap)
                assert lr.mismatches(got, want) == [], (kind, mk, flags, cap)
                assert want[1][3] == (1 if P > cap else 0)
                if P > cap:
                    assert not want[0].any() and want[1][:3] == [0, 0, 0]
                else:
                    assert not want[0][P:].any() and (np.diff((want[0][:P, 0] << 32) | want[0][:P, 1]) > 0).all()


def test_pairs_known_values():
    a = np.array([[[1, 1, 0, 2, -4, 2]]], np.int32)
    b = np.array([[[5, 5, 5, 0, 7, 7]]], np.int32)
    mask = np.array([[[1, 0, 9, 9, 9, 0]]], np.uint8)
    assert lr.pairs_ref(a, b, mask, 0, 4)[0].tolist() == [[1, 5, 2, 1], [2, 7, 1, 0], [0] * 4, [0] * 4]
    p, r = lr.pairs_ref(a, b, mask, 3, 5)
    assert p.tolist() == [[0, 5, 1, 1], [0, 7, 1, 1], [1, 5, 2, 1], [2, 0, 1, 1], [2, 7, 1, 0]] and r == [5, 6, 4, 0]
    assert lr.pairs_ref(a, b, mask, 3, 4)[1] == [0, 0, 0, 1]
    assert lr.pairs_ref(a, a, None, 0, 4)[0][:2].tolist() == [[1, 1, 2, 0], [2, 2, 2, 0]]


@pytest.mark.parametrize("defect", DEFECTS)
def test_planted_defect_is_caught_by_the_gpu_tests_comparison(defect):
    """on small shapes of the GPU test, with its own maps, masks, flags and capacities: at least one case must show the
    defect, and the clean loop must show nothing on the same inputs (test_pairs_restatement_equals_the_triple_loop)"""
    caught = []
    for shape in [(1, 3, 70), (2, 5, 37)]:
        for kind, mk, a, b, mask in _inputs(shape):
            for flags in lr.FLAGS:
                P = lr.pairs_ref(a, b, mask, flags, 1 << 16)[1][0]
                for cap in sorted({max(P, 1), 4096}):
                    if lr.mismatches(brute(a, b, mask, flags, cap, defect), lr.pairs_ref(a, b, mask, flags, cap)):
                        caught.append((shape, kind, mk, flags, cap))
    assert caught, defect
    meant = {"unsorted": "negative", "a0_dropped": "a_empty", "m_over_b": "synthetic", "overflow_at_capacity": "one_pair",
             "run_across_row": "synthetic", "negative_counted": "negative", "m_without_mask_test": "synthetic"}[defect]
    assert any(k[1] == meant for k in caught), (defect, sorted({k[1] for k in caught}))


# ------------------------------------------------------------------------------------------------ the protocols, by hand
def _canvas(*boxes, shape=(1, 12, 24)):
    m = np.zeros(shape, np.uint8)
    for y0, y1, x0, x1 in boxes:
        m[0, y0:y1, x0:x1] = 1
    return m


def test_match_two_lesions_sharing_one_predicted_component():
    truth = _canvas((2, 4, 2, 6), (2, 4, 8, 12))            # two lesions of 8 voxels, a gap of two columns
    pred = _canvas((2, 4, 4, 10))                           # one component of 12: 4 voxels in each
    r = lr.match_ref(pred, truth, min_overlap=0.1)
    # IoU 4 / (12 + 8 - 4) = 0.25 with both: the tie goes to the smaller truth id; one-to-one, so lesion 2 is missed
    assert (r["tp"], r["fp"], r["fn"]) == (1, 0, 1)
    assert r["truth_match"] == [(1, 0.25), (0, 0.0)] and r["pred_match"] == [(1, 0.25)]
    assert r["pred_size"] == [12] and r["truth_size"] == [8, 8]
    assert lr.match_ref(pred, truth, min_overlap=0.26)["tp"] == 0
    d = lr.match_ref(pred, truth, min_overlap=0.4, overlap="dice")          # 2 * 4 / 20 = 0.4
    assert d["tp"] == 1 and d["truth_match"][0] == (1, 0.4)
    assert lr.match_ref(pred, truth, min_overlap=0.99, overlap="any")["tp"] == 1
    w = lr.lesion_wise_ref(pred, truth, 1, dilate_iterations=0)
    # each lesion: gt 8, tp 4, the whole component's 12 voxels in the denominator
    assert [(l["gt"], l["tp"], l["pred"], l["pred_voxels"]) for l in w["lesions"]] == [(8, 4, [1], 12)] * 2
    assert w["fp"] == 0 and w["lesion_dice"] == pytest.approx(2 * 4 / 20, abs=1e-15)
    # dilated once (4-neighbourhood in the plane) the two lesions touch: one lesion, and the prediction is counted once
    w2 = lr.lesion_wise_ref(pred, truth, 1, 1, 6)
    assert [(l["gt"], l["tp"], l["pred_voxels"]) for l in w2["lesions"]] == [(16, 8, 12)]
    assert w2["lesion_dice"] == pytest.approx(16 / 28, abs=1e-15)


def test_one_lesion_split_over_three():
    truth = _canvas((2, 5, 2, 14))                                          # 3 x 12 = 36
    pred = _canvas((2, 5, 2, 5), (2, 5, 6, 9), (2, 5, 10, 16))              # 9, 9, 18 (12 inside)
    r = lr.match_ref(pred, truth, min_overlap=0.1)
    # IoU 9 / 36, 9 / 36, 12 / 42: the largest overlap wins, the other two are false positives
    assert (r["tp"], r["fp"], r["fn"]) == (1, 2, 0)
    assert r["truth_match"] == [(3, 12 / 42)] and r["pred_match"] == [(0, 0.0), (0, 0.0), (1, 12 / 42)]
    w = lr.lesion_wise_ref(pred, truth, 1, dilate_iterations=0)
    assert [(l["gt"], l["tp"], l["pred"], l["pred_voxels"]) for l in w["lesions"]] == [(36, 30, [1, 2, 3], 36)]
    assert w["fp"] == 0 and w["lesion_dice"] == pytest.approx(60 / 72, abs=1e-15)


def test_false_positive_min_size_and_empty_maps():
    truth = _canvas((1, 3, 1, 3), (8, 9, 20, 21))                           # 4 voxels and 1 voxel
    pred = _canvas((1, 3, 1, 3), (5, 7, 10, 12))                            # the first exactly, and a spurious one
    r = lr.match_ref(pred, truth)
    assert (r["tp"], r["fp"], r["fn"]) == (1, 1, 1) and r["truth_match"] == [(1, 1.0), (0, 0.0)]
    w = lr.lesion_wise_ref(pred, truth, 1, dilate_iterations=0)
    assert [l["dice"] for l in w["lesions"]] == [1.0, 0.0] and w["false_positives"] == [2]
    assert w["lesion_dice"] == pytest.approx(1.0 / 3.0, abs=1e-15)
    w = lr.lesion_wise_ref(pred, truth, 1, dilate_iterations=0, min_size=2)
    assert w["dropped"] == [2] and len(w["lesions"]) == 1 and w["lesion_dice"] == pytest.approx(0.5, abs=1e-15)
    # gt counts the voxels of G, not of the dilated lesion: 1 voxel dilated to 5 is still below min_size 2
    assert lr.lesion_wise_ref(pred, truth, 1, 1, 6, min_size=2)["dropped"] == [2]
    # a prediction on a dropped lesion is no false positive
    pred2 = _canvas((1, 3, 1, 3), (8, 9, 20, 21))
    w = lr.lesion_wise_ref(pred2, truth, 1, dilate_iterations=0, min_size=2)
    assert w["fp"] == 0 and w["lesion_dice"] == 1.0
    empty = _canvas()
    assert lr.lesion_wise_ref(empty, empty, 1)["lesion_dice"] == 1.0
    assert lr.lesion_wise_ref(pred, empty, 1)["lesion_dice"] == 0.0 and lr.lesion_wise_ref(empty, truth, 1)["lesion_dice"] == 0.0
    r = lr.match_ref(empty, empty)
    assert (r["tp"], r["fp"], r["fn"]) == (0, 0, 0) and r["truth_match"] == [] and r["pred_size"] == []
    # another class is not a lesion of this one
    assert lr.lesion_wise_ref(pred * 2, truth, 1, dilate_iterations=0)["lesion_dice"] == 0.0


def test_ties_in_the_greedy_order():
    # p1 overlaps t1 and t2 alike (IoU 2 / 12), p2 overlaps t2 more (2 / 10).  The larger overlap goes first whatever the
    # ids: p2 takes t2; of p1's two equal candidates t2 is taken, t1 is left -- both lesions are found.  (4-neighbourhood:
    # p1 and p2 touch across a corner only.)
    truth = _canvas((0, 2, 0, 4), (0, 2, 6, 10))                            # 8 and 8
    pred = _canvas((0, 1, 2, 8), (1, 2, 8, 12))                             # p1: 6 voxels, 2 in t1, 2 in t2; p2: 4 voxels, 2 in t2
    for mode in ("iou", "any"):
        r = lr.match_ref(pred, truth, connectivity=6, min_overlap=0.0, overlap=mode)
        assert r["pred_size"] == [6, 4] and r["truth_size"] == [8, 8]
        assert r["truth_match"] == [(1, 2 / 12), (2, 2 / 10)] and (r["tp"], r["fp"], r["fn"]) == (2, 0, 0)
        assert r["pred_match"] == [(1, 2 / 12), (2, 2 / 10)]
    # under the 8-neighbourhood p1 and p2 are one component of 10 voxels: 2 in t1, 4 in t2
    r = lr.match_ref(pred, truth, min_overlap=0.0)
    assert r["pred_size"] == [10] and r["truth_match"] == [(0, 0.0), (1, 4 / 14)] and (r["tp"], r["fp"], r["fn"]) == (1, 0, 1)
    # without p2, p1's two equal candidates are a tie: the smaller truth id
    r = lr.match_ref(_canvas((0, 1, 2, 8)), truth, min_overlap=0.0)
    assert r["truth_match"] == [(1, 2 / 12), (0, 0.0)] and r["pred_match"] == [(1, 2 / 12)]
    # equal overlaps on one truth lesion: the smaller predicted id
    truth = _canvas((0, 1, 0, 6))
    pred = _canvas((0, 1, 0, 2), (0, 1, 4, 6))
    assert lr.match_ref(pred, truth)["truth_match"] == [(1, 2 / 6)]
    # confidence: the score maximum inside each predicted lesion
    score = np.zeros((1, 12, 24), np.float32)
    score[0, 0, 1], score[0, 0, 5], score[0, 5, 5] = 0.25, 0.75, 0.99
    assert lr.match_ref(pred, truth, score=score)["confidence"] == [np.float32(0.25), np.float32(0.75)]


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


def test_entries_are_declared_exported_and_resolve():
    hdr = open(os.path.join(ROOT, "include", "hdf.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"int64_t\s+hdf_cc_pairs_workspace_bytes\s*\(\s*int64_t\s+capacity\s*\)\s*;", code)
    assert re.search(r"int\s+hdf_cc_pairs\s*\(\s*const\s+int32_t\s*\*\s*ids_a", code)
    assert re.search(r"#define\s+HDF_PAIRS_A0\s+1\b", code) and re.search(r"#define\s+HDF_PAIRS_B0\s+2\b", code)
    import hdf_rt
    from hdf_rt import _lib, lesions
    for name in ("hdf_cc_pairs_workspace_bytes", "hdf_cc_pairs"):
        assert name in _lib.EXPORTS
    for name in ("component_overlap", "match_components", "lesion_wise_scores"):
        assert name in dir(hdf_rt) and callable(getattr(hdf_rt, name))
    assert (lesions.PAIRS_A0, lesions.PAIRS_B0) == (lr.A0, lr.B0)
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(_lib.HdfError):
            hdf_rt.match_components(np.zeros((2, 3, 4), np.uint8), np.zeros((2, 3, 4), np.uint8))
        with pytest.raises(_lib.HdfError):
            hdf_rt.lesion_wise_scores(np.zeros((3, 4), np.uint8), np.zeros((3, 4), np.uint8), 1)
        with pytest.raises(_lib.HdfError):
            hdf_rt.component_overlap(torch.zeros((3, 4), dtype=torch.int32), torch.zeros((3, 4), dtype=torch.int32))


def test_the_shapes_are_cut_to_the_kernels_geometry():
    """the geometry comes from csrc/cc_pairs.h itself (lesion_ref.geometry): rows one voxel longer than a trip, one whole
    span, a last workgroup of seven voxels and one of a single voxel, more pairs than one workgroup sorts or holds in LDS"""
    g = lr.geometry()
    assert g["SPAN"] % g["TRIP"] == 0 and g["SPAN"] > g["TRIP"] >= 64
    vox = [s[0] * s[1] * s[2] for s in lr.SHAPES]
    assert (9, 20, g["TRIP"] + 1) in lr.SHAPES and 9 * 20 * (g["TRIP"] + 1) > g["SPAN"]
    assert g["SPAN"] in vox and g["SPAN"] + 7 in vox and 2 * g["SPAN"] + 1 in vox
    a, b = lr.id_maps(lr.SORT_SHAPE, "synthetic")
    assert lr.pairs_ref(a, b, None, 3, 1 << 16)[1][0] > g["SORT_CHUNK"]
    keys = (a.ravel()[:g["SPAN"]].astype(np.int64) << 32) | b.ravel()[:g["SPAN"]]
    assert len(np.unique(keys)) > g["LDS_SLOTS"]


def test_workspace_size(lib):
    for cap in (0, -1, 65537, 1 << 40):
        assert lib.hdf_cc_pairs_workspace_bytes(cap) == -1 and lib.hdf_last_error().startswith(b"components:")
    for cap in (1, 31, 32, 33, 4096, 4097, 65536):
        slots = (lib.hdf_cc_pairs_workspace_bytes(cap) - 256) // 24
        assert slots >= 2 * cap and slots & (slots - 1) == 0 and (slots < 4 * cap or slots == 64), (cap, slots)
    assert (lib.hdf_cc_pairs_workspace_bytes(4096) - 256) // 24 == 8192       # one workgroup's sort: 8192 keys = 64 KB


def test_entry_refuses_before_launch(lib):
    """HDF_ERR_ARG (1) with a "components:" message.  This host has no device: anything that got as far as a launch would
    come back as HDF_ERR_HIP (2).  Every call here is a refusal, so nothing can launch and the addresses are never
    dereferenced; the accepted forms (ids_a is ids_b, no mask, a mask that aliases an id map, flags 0) run on device memory in
    tests/test_gpu_lesions.py."""
    cap = 8
    need = lib.hdf_cc_pairs_workspace_bytes(cap)
    buf = (C.c_uint8 * (8192 + need))()
    a = (C.addressof(buf) + 63) // 64 * 64
    ia, ib, mask, pairs, res, ws = a, a + 256, a + 512, a + 1024, a + 2048, a + 4096       # 4x4x4: 256, 256, 64; 256; 32

    def call(ia=ia, ib=ib, mask=mask, flags=3, dims=(4, 4, 4), cap=cap, pairs=pairs, res=res, ws=ws, ws_bytes=need):
        return lib.hdf_cc_pairs(ia, ib, mask, flags, *dims, cap, pairs, res, ws, ws_bytes, None)

    def refused(rc, what):
        assert rc == 1 and lib.hdf_last_error().startswith(b"components:"), (what, rc, lib.hdf_last_error())

    for dims in [(0, 4, 4), (4, 1025, 4), (4, 4, -1), (1025, 1, 1)]:
        refused(call(dims=dims, ws_bytes=1 << 40), "dimension %s" % (dims,))
    for c in (0, -3, 65537):
        refused(call(cap=c, ws_bytes=1 << 40), "capacity %d" % c)
    for f in (4, 8, -1, 7):
        refused(call(flags=f), "flags %d" % f)
    for name in ("ia", "ib", "pairs", "res", "ws"):
        refused(call(**{name: None}), "null " + name)
    refused(call(ws_bytes=need - 1), "short workspace")
    refused(call(ws=ws + 4), "workspace not aligned")
    refused(call(pairs=ia + 252), "pairs overlaps ids_a")
    refused(call(pairs=ib - 8), "pairs overlaps ids_b from below")
    refused(call(pairs=mask + 8), "pairs overlaps mask")
    refused(call(res=ia), "result overlaps ids_a")
    refused(call(res=ib + 255), "result overlaps ids_b")
    refused(call(res=mask + 63), "result overlaps mask")
    refused(call(ws=ia - need + 8), "workspace overlaps ids_a")
    refused(call(ws=ib + 248), "workspace overlaps ids_b")
    refused(call(ws=mask + 56), "workspace overlaps mask")
    refused(call(res=pairs + 248), "result overlaps pairs")
    refused(call(ws=pairs + 8), "workspace overlaps pairs")
    refused(call(ws=res - need + 8), "workspace overlaps result")


# ------------------------------------------------------------------------------------------------ the code objects
sys.path.insert(0, os.path.join(ROOT, "tools"))
import codeobj  # noqa: E402

PAIRS_KERNELS = ("pairs_init_kernel", "pairs_voxel_kernel", "pairs_compact_kernel", "pairs_sort_chunk_kernel",
                 "pairs_merge_global_kernel", "pairs_merge_local_kernel", "pairs_rows_kernel")


@pytest.mark.skipif(not os.path.exists(codeobj.LIB), reason="libhdf_hip.so not built")
def test_the_pair_kernels_use_no_scratch():
    ks = codeobj.kernels()
    for fam in PAIRS_KERNELS:
        names = [n for n in ks if fam in n]
        assert names, fam
        for n in names:
            k = ks[n]
            assert not k.get("private_segment_fixed_size", 0) and not k.get("vgpr_spill_count", 0), (n, k)
    assert len([n for n in ks if "pairs_voxel_kernel" in n]) == 2          # with and without a mask
    # the single-workgroup sort holds SORT_CHUNK 64-bit keys in LDS
    sort = [ks[n] for n in ks if "pairs_sort_chunk_kernel" in n][0]
    assert sort["group_segment_fixed_size"] == 8 * 8192 and sort["max_flat_workgroup_size"] == 1024
