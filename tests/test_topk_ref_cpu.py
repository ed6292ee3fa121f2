"""TopKLoss without a GPU: the restatement of tests/topk_ref.py against the reference's recorded vector
(tests/golden/g12_topk_loss.npz, tools/make_topk_goldens.py), the drop-in surface, the refusals of the C entries, the code
objects of the topk_* kernels, the guard-band condition of every case, and the checking functions of
tests/test_gpu_topk_loss.py handed planted defects in place of kernel output -- each must be rejected."""
import ctypes as C
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

import topk_ref as tr
from hdf_rt._lib import BF16, F16, F32
from loss_ref import softmax_a, to_storage

sys.path.insert(0, os.path.join(ROOT, "tools"))
import codeobj  # noqa: E402

PAIRS = [(c, d) for c in tr.CASES for d in tr.DTYPES]
IDS = ["%s-%s" % (c, tr.NAME[d]) for c, d in PAIRS]


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "g12_topk_loss.npz"))


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


# ------------------------------------------------------------------------------------------------ reference and quirks
@pytest.mark.parametrize("case", tr.GOLDEN_CASES)
def test_restatement_equals_the_references_recorded_vector(golden, case):
    x, lab = tr.base_inputs(case)
    assert np.array_equal(golden[case + "_logits"], x.numpy()) and np.array_equal(golden[case + "_labels"], lab.numpy())
    h = tr.held_to(case, F32)
    assert int(golden[case + "_K"]) == h["K"] == tr.topk_count(h["n"], tr.CASES[case][3])
    ref = torch.from_numpy(golden[case + "_topk_desc"].copy())
    assert ref.numel() == h["K"] and bool((ref[:-1] >= ref[1:]).all())
    # the reference's vector is its fp32 evaluation: within the fp32 allowance of the fp64 restatement, element by element
    tr.check_rounded(ref, h["vec64"].sort(descending=True).values, F32, h["acc_v"], "golden vector")


def test_the_quirks_hold(golden):
    """the golden was recorded from TopKLoss(reduction='mean'): a K-vector all the same; ours keeps that"""
    from loss.cross_entropy import TopKLoss
    cases = json.loads(str(golden["cases"]))
    assert sorted(cases) == sorted(tr.GOLDEN_CASES)
    for case in tr.GOLDEN_CASES:
        assert golden[case + "_topk_desc"].shape == (int(golden[case + "_K"]),)
    t = torch.zeros(1, 2, 4, 4)
    for red in (None, "mean", "sum"):
        assert TopKLoss(reduction=red)._spec(t)[4] is False          # the vector form
    assert TopKLoss(reduction="topk")._spec(t)[4] is True
    assert TopKLoss()._spec(t)[1:4] == (None, -100, 10)


def test_dropin_surface():
    from hdf_rt import _lib
    from loss.combine_loss import DeepSuperloss
    from loss.cross_entropy import TopKLoss
    with pytest.raises(ValueError):
        TopKLoss(weight=[1.0, -0.5])
    with pytest.raises(ValueError):
        TopKLoss(weight=torch.tensor([1.0, -0.5]))
    with pytest.raises(ValueError):
        TopKLoss(reduction="median")
    with pytest.raises(ValueError):
        TopKLoss(ignore_index=-1)
    x, t = torch.zeros(1, 3, 4, 4, 4), torch.zeros(1, 3, 4, 4, 4)
    # K == 0 (64 voxels, k = 1): the vector forms return an empty tensor without a launch, 'topk' would be the mean of none
    for red in (None, "mean", "sum"):
        out = TopKLoss(k=1, reduction=red)(x, t)
        assert out.shape == (0,) and out.dtype == torch.float32
    xg = x.clone().requires_grad_(True)
    TopKLoss(k=1)(xg, t).sum().backward()
    assert xg.grad.shape == x.shape and float(xg.grad.abs().max()) == 0.0
    with pytest.raises(ValueError):
        TopKLoss(k=1, reduction="topk")(x, t)
    with pytest.raises(ValueError):                        # ignore_index beyond the classes
        TopKLoss(ignore_index=3)(x, t)
    with pytest.raises(AssertionError):
        TopKLoss()(x, torch.zeros(1, 3, 4, 4, 8))
    with pytest.raises(_lib.HdfError, match="depth 1"):     # depth 1 means 2-D to the kernels: no 3-D target of depth 2
        from hdf_rt.loss_fn import TopKVoxelCE
        TopKVoxelCE.apply(TopKLoss()._spec(torch.zeros(1, 3, 2, 8, 8), 1), torch.zeros(1, 3, 1, 4, 4))
    assert not hasattr(TopKLoss(), "_check")               # settings are checked once, when the module is built
    with pytest.raises(_lib.HdfError):                     # K = 6 voxels and no GPU: no fallback
        TopKLoss()(x, t)
    # DeepSuperloss: the vector form is refused with a pointer to reduction='topk', the scalar form is dispatched
    with pytest.raises(NotImplementedError, match="reduction='topk'"):
        DeepSuperloss(criterion=TopKLoss())([x], t)
    with pytest.raises(_lib.HdfError):
        DeepSuperloss(criterion=TopKLoss(reduction="topk"))([x, torch.zeros(1, 3, 2, 2, 2)], t)


def test_c_entries_refuse_before_any_launch(lib):
    """HDF_ERR_ARG (1) with a message starting "topk:"; on this host, which has no device, a launch or a memset would come
    back as HDF_ERR_HIP (2).  The addresses are never dereferenced."""
    from hdf_rt import _lib
    buf = (C.c_float * 64)()
    a = C.addressof(buf)
    big = 1 << 40

    def refused(rc, what):
        assert rc == 1 and lib.hdf_last_error().startswith(b"topk:"), (what, rc, lib.hdf_last_error())

    assert lib.hdf_loss_topk_workspace_bytes(2, 128, 128, 128) == 65536 + 8 * 2 * 128 ** 3
    assert lib.hdf_loss_topk_workspace_bytes(1, 1, 3, 5) == 65536 + 2 * 256
    assert lib.hdf_loss_topk_workspace_bytes(1, 2048, 1024, 1024) == -1 and lib.hdf_loss_topk_workspace_bytes(0, 8, 8, 8) == -1
    sel = lib.hdf_op_topk_select
    refused(sel(a, 64, 0, a, big, a, a, a, a, None), "K < 1")
    refused(sel(a, 64, 65, a, big, a, a, a, a, None), "K > n")
    refused(sel(a, 1 << 31, 5, a, big, a, a, a, a, None), "n >= 2^31")
    refused(sel(a, 64, 5, a, 65535, a, a, a, a, None), "small workspace")
    fwd, bwd = lib.hdf_loss_topk_forward, lib.hdf_loss_topk_backward
    ok = dict(dtype=_lib.F32, b=1, c=3, d=4, h=4, w=4, s=0, ign=-100, K=6, wsb=big, outs=(a, None))
    bad = {"K < 1": dict(K=0), "K > n": dict(K=65), "n >= 2^31": dict(d=2048, h=1024, w=1024), "one class": dict(c=1),
           "nine classes": dict(c=9), "scale_shift 4": dict(s=4), "scale_shift -1": dict(s=-1), "ignore -1": dict(ign=-1),
           "ignore == n_cls": dict(ign=3), "batch above the grid's rows": dict(b=65536, d=1, h=1, w=4), "small workspace": dict(wsb=65536 + 511), "both": dict(outs=(a, a)),
           "neither": dict(outs=(None, None))}
    for what, change in bad.items():
        q = dict(ok, **change)
        for dtype in (_lib.F32, _lib.BF16, _lib.F16):
            geom = (dtype, a, a, q["b"], q["c"], q["d"], q["h"], q["w"], q["s"], None, q["ign"], q["K"], a, q["wsb"])
            refused(fwd(*geom, q["outs"][0], q["outs"][1], None), "forward: " + what)
            refused(bwd(*geom, q["outs"][0], q["outs"][1], a, None), "backward: " + what)


def test_topk_kernels_have_no_scratch_and_no_register_spills(lib):
    ks = {n: k for n, k in codeobj.kernels().items() if n.startswith("topk_")}
    for fam in ("topk_ce_kernel", "topk_hist_kernel", "topk_pick_kernel", "topk_count_kernel", "topk_scan_kernel",
                "topk_write_kernel", "topk_mean_kernel", "topk_bwd_kernel"):
        assert any(n.startswith(fam) for n in ks), fam
    for T in ("float", "bf16_t", "f16_t"):
        for vec in (1, 4):
            for mc in (4, 8):
                assert "topk_ce_kernel<%s, %d, %d>" % (T, vec, mc) in ks and "topk_bwd_kernel<%s, %d, %d>" % (T, vec, mc) in ks
    bad = {n: (k.get("private_segment_fixed_size", 0), k.get("vgpr_spill_count", 0)) for n, k in ks.items()
           if k.get("private_segment_fixed_size", 0) or k.get("vgpr_spill_count", 0)}
    assert not bad, bad
    scalar = {n: k.get("sgpr_spill_count", 0) for n, k in ks.items() if k.get("sgpr_spill_count", 0)}
    assert not scalar, scalar


# ------------------------------------------------------------------------------------------------ the band condition
@pytest.mark.parametrize("case,dtype", PAIRS, ids=IDS)
def test_guard_band_holds_at_most_eight_voxels(case, dtype):
    h = tr.held_to(case, dtype)
    band = int(h["band"].sum())
    print("%s %s: n %d K %d T64 %.9g acc_v %.3g band %d exact ties %d" % (case, tr.NAME[dtype], h["n"], h["K"], h["T64"],
                                                                         h["acc_v"], band, h["ties"]))
    assert 1 <= band <= tr.BAND_CAP            # (the K-th largest voxel itself is always inside)
    assert 0.0 < h["acc_v"] < 1e-3 * max(1.0, h["T64"])
    assert h["K"] >= 1 and int((h["rank64"] >= 0).sum()) == h["K"]


# ------------------------------------------------------------------------------------------------ planted defects
def faultless(case, dtype, mean):
    """what a faultless kernel returns, formed from the restatement: (h, res, rank, vector, mean, dlogits, g)"""
    h = tr.held_to(case, dtype)
    g = tr.upstream(h, mean)
    res = h["res64"].float()
    rank = h["rank64"]
    x, onehot, _ = tr.inputs(case, dtype)
    gvox = tr.per_voxel_upstream(h, rank, g, mean)
    g64 = tr.gradient(x, onehot, tr.case_weight(case), tr.case_ignore(case), softmax_a(x)[0], gvox)
    return h, res, rank, res[rank >= 0], np.float32(h["mean64"]), to_storage(g64, dtype), g


def run_checks(h, res, rank, vec, mean, dl, g, mean_form):
    tr.check_selection(h, rank)
    tr.check_own_selection(res.numpy(), rank.numpy())
    tr.check_vector(h, vec, res, rank)
    tr.check_mean(h, mean)
    tr.check_grad(h, dl, rank, g, mean_form)


@pytest.mark.parametrize("case,dtype,mean", [("small_odd", F32, True), ("weighted_k50", BF16, False), ("ignore0", F16, True),
                                             ("c8_k1", F32, False)])
def test_the_faultless_restatement_passes_every_check(case, dtype, mean):
    run_checks(*faultless(case, dtype, mean), mean)


def test_defect_k_taken_with_ceil():
    h, res, _rank, *_ = faultless("small_odd", F32, True)
    k_ceil = math.ceil(h["n"] * tr.CASES["small_odd"][3] / 100)
    assert k_ceil == h["K"] + 1
    rank = torch.from_numpy(tr.select(h["res64"].numpy(), k_ceil)[3])
    with pytest.raises(AssertionError, match="selected"):
        tr.check_selection(h, rank)


def test_defect_class_weight_applied_after_the_selection():
    case = "weighted_k50"
    h = tr.held_to(case, F32)
    x, onehot, _ = tr.inputs(case, F32)
    unweighted = tr.per_voxel(x, onehot, None, tr.case_ignore(case))
    rank = torch.from_numpy(tr.select(unweighted.numpy(), h["K"])[3])
    with pytest.raises(AssertionError, match="outside the guard band"):
        tr.check_selection(h, rank)
    w = tr.case_weight(case)[onehot.argmax(1).flatten()]
    with pytest.raises(AssertionError):
        tr.check_vector(h, (unweighted * w)[rank >= 0].float(), (unweighted * w).float(), rank)


def test_defect_ignored_voxels_dropped_from_the_voxel_count():
    case = "ignore0"
    h = tr.held_to(case, F32)
    _x, _onehot, lab = tr.inputs(case, F32)
    k_short = tr.topk_count(int((lab != tr.case_ignore(case)).sum()), tr.CASES[case][3])
    assert 1 <= k_short < h["K"]
    rank = torch.from_numpy(tr.select(h["res64"].numpy(), k_short)[3])
    with pytest.raises(AssertionError, match="selected"):
        tr.check_selection(h, rank)


def quantised(n, seed=5):
    """values on 7 levels: thousands of ties at any threshold"""
    return (torch.randint(0, 7, (n,), generator=torch.Generator().manual_seed(seed)).float() * 0.25).numpy()


def test_defect_last_tie_taken_instead_of_the_first():
    v, K = quantised(20000), 2000
    good, bad = tr.select_exact(v, K), tr.select_exact(v, K, last_tie=True)
    assert good["result"] == bad["result"] and good["result"][2] > 100 and not np.array_equal(good["rank"], bad["rank"])
    tr.check_select_exact(v, K, good["result"], good["rank"], good["values_out"], np.float32(good["mean64"]))
    with pytest.raises(AssertionError, match="rank"):
        tr.check_select_exact(v, K, bad["result"], bad["rank"], bad["values_out"], np.float32(bad["mean64"]))
    with pytest.raises(AssertionError, match="exact selection"):
        tr.check_own_selection(v, bad["rank"])


def test_defect_gradient_divided_by_n_instead_of_k():
    case, dtype = "small_odd", BF16
    h, res, rank, vec, mean, dl, g = faultless(case, dtype, True)
    tr.check_grad(h, dl, rank, g, True)
    with pytest.raises(AssertionError, match="selected voxels"):
        tr.check_grad(h, to_storage(dl.double() * h["K"] / h["n"], dtype), rank, g, True)


def test_defect_selected_gradient_written_for_an_unselected_voxel_inside_the_band():
    """inside the band either selection is allowed -- but the gradient must follow the selection the kernel made"""
    found = None
    for case, dtype in PAIRS:
        h = tr.held_to(case, dtype)
        cand = torch.nonzero(h["band"] & (h["rank64"] < 0)).flatten()
        if cand.numel():
            found = (case, dtype, int(cand[0]))
            break
    assert found, "no case has an unselected voxel inside its guard band"
    case, dtype, v = found
    h, res, rank, vec, mean, dl, g = faultless(case, dtype, True)
    x, onehot, _ = tr.inputs(case, dtype)
    # the gradient this voxel would have, were it selected
    gvox = torch.zeros(h["n"], dtype=torch.float64)
    gvox[v] = float(g) / h["K"]
    extra = tr.gradient(x, onehot, tr.case_weight(case), tr.case_ignore(case), softmax_a(x)[0], gvox)
    assert float(extra.abs().max()) > 0.0
    with pytest.raises(AssertionError, match="not \\+0"):
        tr.check_grad(h, to_storage(dl.double() + extra, dtype), rank, g, True)
    # the allowed alternative: the band voxel selected INSTEAD of the K-th largest one, and the gradient along with it
    kth = int(torch.nonzero((h["rank64"] >= 0) & (h["res64"] == h["T64"])).flatten()[-1])
    sel = h["rank64"] >= 0
    sel[kth], sel[v] = False, True
    rank2 = torch.where(sel, torch.cumsum(sel, 0) - 1, torch.full_like(h["rank64"], -1)).int()
    tr.check_selection(h, rank2)
    gvox2 = tr.per_voxel_upstream(h, rank2, g, True)
    dl2 = to_storage(tr.gradient(x, onehot, tr.case_weight(case), tr.case_ignore(case), softmax_a(x)[0], gvox2), dtype)
    tr.check_grad(h, dl2, rank2, g, True)
