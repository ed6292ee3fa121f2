"""The two-class losses without a GPU: an fp64 restatement of the reference's FocalLoss / FLPlusDice / DeepSuperloss
(loss/cross_entropy.py:45-73, loss/combine_loss.py:37-79, loss/dice_loss.py:5-87), pinned here to the reference's own
values (tests/golden/g11_focal_loss.npz, tools/make_focal_goldens.py) and used by tests/test_gpu_focal_loss.py as the
yardstick of the fused kernels; the drop-in constructors; the code objects of the focal kernels."""
import inspect
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT

# ---------------------------------------------------------------------------------------------- fp64 restatement


def _bce_terms(p, t):
    """F.binary_cross_entropy (both logs clamped at -100) and 1 - p_t"""
    bce = -(t * torch.clamp(torch.log(p), min=-100.0) + (1 - t) * torch.clamp(torch.log(1 - p), min=-100.0))
    return bce, 1 - (p * t + (1 - p) * (1 - t))


def _alpha_t(t, alpha):
    return alpha * t + (1 - alpha) * (1 - t) if alpha >= 0 else torch.ones_like(t)


def focal_map(p, t, alpha, gamma):
    bce, q = _bce_terms(p, t)
    return _alpha_t(t, alpha) * bce * (q ** gamma if gamma != 0 else torch.ones_like(q))


def focal_dp(p, t, alpha, gamma):
    """d focal / d p as torch's autograd takes it: BCE backward (p - t) / max(p (1-p), 1e-12), pow backward 0 at gamma 0"""
    bce, q = _bce_terms(p, t)
    d = (q ** gamma if gamma != 0 else torch.ones_like(q)) * (p - t) / torch.clamp(p * (1 - p), min=1e-12)
    if gamma != 0:
        d = d + bce * gamma * q ** (gamma - 1) * (1 - 2 * t)
    return _alpha_t(t, alpha) * d


def dice_loss(p, t, weight=None, ignore=0):
    """DiceLoss(weight, ignore_index) on probabilities p (BinaryDiceLoss defaults: smooth 1e-5, p 1, batch mean)"""
    c = t.shape[1]
    total = 0.0
    for i in range(c):
        if i == ignore:
            continue
        pi, ti = p[:, i].reshape(p.shape[0], -1), t[:, i].reshape(t.shape[0], -1)
        d = (1 - (2 * (pi * ti).sum(1) + 1e-5) / ((pi + ti).sum(1) + 1e-5)).mean()
        total = total + (d * float(weight[i]) if weight is not None else d)
    return total / (c - 1 if ignore is not None else c)


def spec_of(case):
    """case record of g11_focal_loss -> (w_focal, alpha, gamma, reduction, w_dice, weight, ignore)"""
    if case["kind"] == "focal":
        return (1.0, float(case["alpha"]), float(case["gamma"]), case["red"], 0.0, None, 0)
    return (1.0, 1.0, 2.0, "mean", 1.0, case["weight"], case["ignore"])


def restated(outs, target, spec):
    """sum_i 2^-i (w_focal * Focal + w_dice * Dice)(out_i, target nearest-downsampled to out_i) in fp64 -> (loss,
    [dL/dout_i]).  The focal term takes the fp32 softmax; everything after it is fp64."""
    w_focal, alpha, gamma, red, w_dice, weight, ignore = spec
    t0 = torch.as_tensor(target).double()
    total, grads = 0.0, []
    for i, o in enumerate(outs):
        s = 1 << i
        t = t0[(slice(None), slice(None)) + (slice(None, None, s),) * (t0.dim() - 2)]
        z = torch.as_tensor(o).detach().double().requires_grad_(True)
        p = torch.softmax(z, 1)
        # the focal term on the softmax rounded to fp32, as the reference (and the kernels) evaluate it: 1 - p of a p
        # near 1 (the log clamp, BCE's floor) is decided by that rounding
        pd = torch.softmax(z.detach().float(), 1).double()
        den = float(pd.numel()) if red == "mean" else 1.0
        lf = focal_map(pd, t, alpha, gamma).sum() / den
        gp = focal_dp(pd, t, alpha, gamma) / den
        w = 1.0 / s
        gz = w * w_focal * pd * (gp - (gp * pd).sum(1, keepdim=True))   # softmax backward on the same p
        if w_dice:
            ld = dice_loss(p, t, weight, ignore)
            (w * w_dice * ld).backward()
            gz = gz + z.grad
            total += w * w_dice * float(ld.detach())
        total += w * w_focal * float(lf)
        grads.append(gz)
    return total, grads


def g11():
    g = np.load(os.path.join(GOLDEN, "g11_focal_loss.npz"), allow_pickle=False)
    return g, json.loads(str(g["cases"]))


def case_inputs(g, tag, case):
    outs = [torch.from_numpy(g[f"{tag}_logits{i}"]) for i in range(case["n"])]
    return outs, torch.from_numpy(g[f"{tag}_target"].astype(np.float32))


def rl2(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


# ------------------------------------------------------------------------------------------------------------ tests

G11, CASES = g11()


@pytest.mark.parametrize("tag", list(CASES))
def test_restatement_matches_the_reference(tag):
    case = CASES[tag]
    outs, t = case_inputs(G11, tag, case)
    loss, grads = restated(outs, t, spec_of(case))
    ref = float(G11[f"{tag}_loss"])
    assert abs(loss - ref) <= 1e-5 * abs(ref), (loss, ref)
    for i, gr in enumerate(grads):
        assert rl2(gr, G11[f"{tag}_grad{i}"]) <= 1e-5, i


def test_restatement_reproduces_the_saturated_voxels():
    """the issue's table: gaps 5, 20, 28, 40, 200, -40 (row 0: the other class leads; row 1: the target leads).  The
    1e-12 floor of BCE's backward gives -0.69 at gap 28 and -4.2e-6 at 40; the log clamp gives a loss of 100 at 200."""
    outs, t = case_inputs(G11, "sat", CASES["sat"])
    _, (gr,) = restated(outs, t, spec_of(CASES["sat"]))
    ref = G11["sat_grad0"]
    assert np.abs(gr.numpy() - ref).max() <= 1e-6
    np.testing.assert_allclose(ref[0, 1, 0], [-1.04618, -1.0000001, -0.69144, -4.2484e-6, 0.0, 0.0], rtol=1e-4, atol=1e-9)
    per_voxel = focal_map(torch.softmax(outs[0].double(), 1), t.double(), 1.0, 2.0).sum(1)[0, 0]
    np.testing.assert_allclose(per_voxel.numpy(), [4.93992, 20.0, 28.0, 40.0, 100.0, 0.0], rtol=1e-5, atol=1e-12)


def test_dropins_keep_the_reference_constructors():
    from loss.combine_loss import DeepSuperloss, FLPlusDice
    from loss.cross_entropy import FocalLoss
    sig = inspect.signature(FocalLoss.__init__)
    assert [(k, v.default) for k, v in sig.parameters.items()][1:] == [("alpha", 1), ("gamma", 2), ("num_classes", 2),
                                                                        ("reduction", "sum")]
    sig = inspect.signature(FLPlusDice.__init__)
    assert [(k, v.kind) for k, v in sig.parameters.items()][1:] == [
        ("weight", inspect.Parameter.POSITIONAL_OR_KEYWORD), ("ignore_index", inspect.Parameter.POSITIONAL_OR_KEYWORD),
        ("kwargs", inspect.Parameter.VAR_KEYWORD)]
    assert sig.parameters["weight"].default is None and sig.parameters["ignore_index"].default is None
    fl = FocalLoss()
    assert (fl.alpha, fl.gamma, fl.num_classes, fl.reduction) == (1, 2, 2, "sum")
    FocalLoss(alpha=0.25, gamma=0, reduction="mean")
    FocalLoss(alpha=-1, gamma=3)
    FLPlusDice(weight=torch.tensor([1.0, 2.0]), ignore_index=0, p=1)
    DeepSuperloss(criterion=FocalLoss(reduction="sum"))


@pytest.mark.parametrize("kw", [dict(reduction="none"), dict(reduction=None), dict(gamma=0.5), dict(gamma=-1),
                                dict(gamma=0.999)])
def test_focal_settings_the_kernels_do_not_implement_raise_at_construction(kw):
    from loss.cross_entropy import FocalLoss
    with pytest.raises(NotImplementedError):
        FocalLoss(**kw)


def test_flplusdice_rejects_other_dice_settings_at_construction():
    from loss.combine_loss import FLPlusDice
    with pytest.raises(NotImplementedError):
        FLPlusDice(weight=None, ignore_index=0, p=2)


def test_the_fused_focal_loss_has_no_cpu_fallback():
    from hdf_rt import _lib
    from loss.combine_loss import DeepSuperloss
    from loss.cross_entropy import FocalLoss
    with pytest.raises(_lib.HdfError):
        DeepSuperloss(criterion=FocalLoss())([torch.zeros(1, 2, 8, 8)], torch.zeros(1, 2, 8, 8))


sys.path.insert(0, os.path.join(ROOT, "tools"))
import codeobj  # noqa: E402


@pytest.mark.skipif(not os.path.exists(codeobj.LIB), reason="libhdf_hip.so not built")
def test_focal_kernels_have_no_scratch_and_no_spills():
    """the two per-voxel passes (3 storage types x 4 / 8 class slots each), gated like loss_fwd_kernel / loss_bwd_kernel
    in test_cpu_codeobject.py; the one-block finalize shares the CE finalize's body and its frame"""
    ks = codeobj.kernels()
    for family in ("focal_fwd_kernel", "focal_bwd_kernel"):
        fam = {n: k for n, k in ks.items() if n.startswith(family)}
        assert len(fam) == 6, sorted(fam)
        bad = {n: (k.get("private_segment_fixed_size", 0), k.get("vgpr_spill_count", 0)) for n, k in fam.items()
               if k.get("private_segment_fixed_size", 0) or k.get("vgpr_spill_count", 0)}
        assert not bad, bad
    fin, ce = ks["focal_finalize_kernel"], ks["loss_finalize_kernel"]
    assert fin.get("vgpr_spill_count", 0) == 0
    assert fin.get("private_segment_fixed_size", 0) <= ce.get("private_segment_fixed_size", 0)
