"""GPU parity of the two-class losses (hdf_loss_focal_*; reference loss/cross_entropy.py:45-73, loss/combine_loss.py:37-79)
through the drop-in FocalLoss / FLPlusDice / DeepSuperloss: against the reference's own values (g11_focal_loss,
g11_focal_2d_train) and against the fp64 restatement of tests/test_focal_loss_cpu.py (pinned there to the reference) on
16-bit logits, odd geometries and soft targets."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import GOLDEN  # noqa: E402
from oracle import detgen  # noqa: E402
from oracle import hdf_oracle as orc  # noqa: E402
from test_focal_loss_cpu import CASES, G11, case_inputs, restated, rl2, spec_of  # noqa: E402
from test_gpu_bench_geometry import _check_adam_vs_fixture, _check_grads_vs_fixture, _rel  # noqa: E402
from test_gpu_model_2d import _build as _build_2d, _data as _data_2d  # noqa: E402

DEV = "cuda:0"


def _criterion(case):
    from loss.combine_loss import DeepSuperloss, FLPlusDice
    from loss.cross_entropy import FocalLoss
    if case["kind"] == "focal":
        crit = FocalLoss(alpha=case["alpha"], gamma=case["gamma"], reduction=case["red"])
    else:
        w = None if case["weight"] is None else torch.tensor(case["weight"])
        crit = FLPlusDice(weight=w, ignore_index=case["ignore"])
    return DeepSuperloss(criterion=crit) if case["deep"] else crit


def _run(crit, outs, t, deep):
    outs = [o.detach().to(DEV).requires_grad_(True) for o in outs]
    loss = crit(outs, t.to(DEV)) if deep else crit(outs[0], t.to(DEV))
    loss.backward()
    torch.cuda.synchronize()
    return loss, [o.grad for o in outs]


def _node(outs, t, spec):
    """the autograd node itself: spec = (w_focal, alpha, gamma, reduction, w_dice, class_weight, ignore_index)"""
    from hdf_rt.loss_fn import DeepSuperFocalDice
    outs = [o.requires_grad_(True) for o in outs]
    loss = DeepSuperFocalDice.apply((t,) + tuple(spec), *outs)
    loss.backward()
    torch.cuda.synchronize()
    return loss, [o.grad for o in outs]


# ------------------------------------------------------------------------------------ (a) the reference's values


@pytest.mark.parametrize("tag", list(CASES))
def test_dropins_match_the_reference_fp32(tag):
    case = CASES[tag]
    outs, t = case_inputs(G11, tag, case)
    loss, grads = _run(_criterion(case), outs, t, case["deep"])
    assert loss.dtype == torch.float32 and loss.dim() == 0
    ref = float(G11[f"{tag}_loss"])
    print(f"  {tag}: loss {loss.item():.6f} ref {ref:.6f}")
    assert abs(loss.item() - ref) <= 2e-5 * abs(ref)
    for i, gr in enumerate(grads):
        assert gr.dtype == torch.float32
        e = rl2(gr, G11[f"{tag}_grad{i}"])
        print(f"    dlogits{i} rel-l2 {e:.2e}")
        assert e <= 1e-4, i
    if tag == "sat":      # the saturated voxels element by element (BCE's 1e-12 floor, the log clamp at 100)
        d = np.abs(grads[0].cpu().numpy() - G11["sat_grad0"]).max()
        print(f"    saturated voxels: max |d dlogits| {d:.2e}")
        assert d <= 1e-5


# ------------------------------------------------------------------------------------ (b) 16-bit logits


@pytest.mark.parametrize("dtype,tol", [(torch.bfloat16, 1e-2), (torch.float16, 2e-3)], ids=["bf16", "fp16"])
@pytest.mark.parametrize("tag", ["deep3_c2", "deep3_c4", "deep2_c2", "am1_g3", "soft_c3"])
def test_16bit_logits_against_the_restatement(tag, dtype, tol):
    case = CASES[tag]
    outs, t = case_inputs(G11, tag, case)
    outs = [o.to(dtype) for o in outs]
    loss, grads = _run(_criterion(case), outs, t, case["deep"])
    ref, rg = restated([o.float() for o in outs], t, spec_of(case))
    el = abs(loss.item() - ref) / abs(ref)
    eg = max(rl2(g.float(), r) for g, r in zip(grads, rg))
    print(f"  {tag} {dtype}: loss rel {el:.2e}, dlogits rel-l2 {eg:.2e}")
    assert all(g.dtype == dtype for g in grads)
    assert el <= 1e-4
    assert eg <= tol


# ------------------------------------------------------------------------------------ (c) geometry sweep

# (spatial of scale 0, n_cls, scales, soft target, unaligned views, (w_focal, alpha, gamma, reduction, w_dice, weight, ignore))
SWEEP = [
    ((8, 16, 24), 2, 4, False, False, (1.0, 1.0, 2.0, "sum", 0.0, None, 0)),
    ((8, 8, 12), 5, 3, True, False, (1.0, 0.25, 2.0, "sum", 0.0, None, 0)),
    ((40, 24), 3, 4, False, True, (1.0, 1.0, 2.0, "mean", 1.0, None, 0)),
    ((16, 20), 8, 2, True, True, (1.0, -1.0, 1.0, "sum", 0.0, None, 0)),
    ((12, 36), 2, 1, False, False, (1.0, 0.25, 0.0, "sum", 0.0, None, 0)),
    ((4, 8, 8), 8, 1, False, True, (1.0, 0.5, 3.0, "mean", 1.0, [0.5, 1, 2, 1, 1, 1, 0.2, 3], None)),
    ((8, 12, 20), 3, 2, True, True, (1.0, 1.0, 1.5, "sum", 0.0, None, 0)),
    ((32, 64), 2, 4, False, False, (1.0, 1.0, 2.0, "mean", 1.0, [0.3, 1.7], 0)),
]


def _unaligned(x):
    """the same values in a contiguous view 4 bytes off a 16-byte boundary (the kernels' 1-voxel form)"""
    buf = torch.empty(x.numel() + 1, dtype=x.dtype, device=DEV)
    v = buf[1:].view(x.shape)
    v.copy_(x)
    assert v.data_ptr() % 16 != 0
    return v


@pytest.mark.parametrize("k", range(len(SWEEP)))
def test_geometry_sweep_against_the_restatement(k):
    sp, c, n, soft, unal, spec = SWEEP[k]
    g = torch.Generator().manual_seed(500 + k)
    if soft:
        t = torch.rand((2, c) + sp, generator=g)
    else:
        t = torch.nn.functional.one_hot(torch.randint(0, c, (2,) + sp, generator=g), c).movedim(-1, 1).float()
    outs = [torch.randn((2, c) + tuple(s >> i for s in sp), generator=g) * 2.5 for i in range(n)]
    dev = [o.to(DEV) for o in outs]
    td = t.to(DEV)
    if unal:
        dev, td = [_unaligned(o) for o in dev], _unaligned(td)
    loss, grads = _node(dev, td, spec)
    ref, rg = restated(outs, t, spec)
    el = abs(loss.item() - ref) / abs(ref)
    eg = max(rl2(a, b) for a, b in zip(grads, rg))
    print(f"  {sp} C={c} scales={n} soft={soft} unaligned={unal} {spec[1:4]}: loss rel {el:.2e} dlogits rel-l2 {eg:.2e}")
    assert el <= 2e-5
    assert eg <= 1e-4


# ------------------------------------------------------------------------------------ (d) reproducibility, (e) Dice


def test_two_calls_are_bit_identical():
    case = CASES["deep3_c4"]
    outs, t = case_inputs(G11, "deep3_c4", case)
    l1, g1 = _run(_criterion(case), outs, t, True)
    l2, g2 = _run(_criterion(case), outs, t, True)
    assert l1.item() == l2.item()
    assert all(torch.equal(a, b) for a, b in zip(g1, g2))


@pytest.mark.parametrize("cw,ign", [(None, 0), ([0.2, 1.0, 2.5, 0.6], 0), (None, None)])
def test_dice_term_is_the_weighted_loss_dice(cw, ign):
    """focal_weight 0 against hdf_loss_weighted_* with ce_weight 0: the Dice arithmetic is shared"""
    from hdf_rt.loss_fn import DeepSuperCEDice
    outs, t = case_inputs(G11, "deep3_c4", CASES["deep3_c4"])
    w = None if cw is None else torch.tensor(cw)
    lf, gf = _node([o.to(DEV) for o in outs], t.to(DEV), (0.0, 1.0, 2.0, "sum", 1.0, w, ign))
    oc = [o.to(DEV).requires_grad_(True) for o in outs]
    lc = DeepSuperCEDice.apply((t.to(DEV), 0.0, 1.0, w, ign), *oc)
    lc.backward()
    assert abs(lf.item() - lc.item()) <= 1e-6 * abs(lc.item())
    for a, o in zip(gf, oc):
        assert rl2(a, o.grad) <= 1e-6


# ------------------------------------------------------------------------------------ (f) the 2-D model's train step


def _without_dead_tensors(g):
    """the fixture with the sampled gradients of its dead tensors (the conv biases ahead of an InstanceNorm, under
    1e-6 of the total gradient norm: rounding noise, which _check_grads_vs_fixture skips the same way) set to zero.  Under
    FocalLoss('sum') that noise is thousands of times the CE-mean fixture's and clears the absolute 2e-6 floor by which
    _check_adam_vs_fixture tells live entries from noise; zeroed, those no-decay entries drop out of its count."""
    d = {k: g[k] for k in g.files}
    dead = d["grad_norms"] < 1e-6 * np.sqrt((d["grad_norms"] ** 2).sum())
    d["grad_samples"] = np.where(dead[:, None], 0.0, d["grad_samples"])
    return d


def test_2d_train_step_vs_reference_golden():
    """the shipped two-class configuration (HDenseFormer_2D_32 with DeepSuperloss(FocalLoss('sum'))) at a small
    geometry: fp32 with the checks of test_gpu_model_2d.py::test_2d_train_step_vs_reference_golden, then bf16"""
    from loss.combine_loss import DeepSuperloss
    from loss.cross_entropy import FocalLoss
    g = np.load(os.path.join(GOLDEN, "g11_focal_2d_train.npz"), allow_pickle=False)
    in_ch, n_cls, nf, td = [int(v) for v in g["cfg"][:4]]
    cfg = (in_ch, n_cls, nf, tuple(int(v) for v in g["cfg"][4:]), td)
    batch, seed = int(g["batch"]), int(g["train_seed"])
    x, onehot = _data_2d(cfg, batch, "g11_focal_2d_train")
    crit = DeepSuperloss(criterion=FocalLoss(reduction="sum"))
    res = {}
    for dtype in ("fp32", "bf16"):
        net, sd = _build_2d(cfg, dtype)
        net.train()
        net.set_dropout_seed(seed)
        outs = net(x.to(DEV))
        loss = crit(outs, onehot.to(DEV))
        loss.backward()
        torch.cuda.synchronize()
        ref = float(g["loss"])
        print(f"  {dtype}: loss {loss.item():.4f} ref {ref:.4f}")
        res[dtype] = torch.cat([p.grad.flatten().cpu() for _, p in net.named_parameters()]).double()
        if dtype == "fp32":
            for i in range(4):
                s = max(1, int(g["sample_step"]) >> i)
                e = _rel(outs[i].detach()[:, :, ::s, ::s], torch.from_numpy(g[f"out{i}"]))
                print(f"  out{i} rel {e:.3e}")
                assert e < 1e-3
            assert abs(loss.item() - ref) < 1e-4 * max(1.0, abs(ref))
            _check_grads_vs_fixture(g, net, 2e-2, 5e-2, tight=("conv1x1.weight",))
            _check_adam_vs_fixture(_without_dead_tensors(g), net, min_live=1500)
        else:
            assert outs[0].dtype == torch.bfloat16
            assert abs(loss.item() - ref) < 3e-2 * abs(ref)
    a, b = res["bf16"], res["fp32"]
    cos = float((a @ b) / (a.norm() * b.norm()))
    print("  bf16 vs fp32 whole-gradient cosine", cos)
    assert cos >= 0.98


# ------------------------------------------------------------------------------------ (g) through the 3-D model


def test_flplusdice_gradients_through_the_3d_model_match_the_restatement():
    """g1-tiny with DeepSuperloss(FLPlusDice(None, 0)): the fused path's parameter gradients against those of the
    restatement's fp64 dlogits backpropagated through the same model"""
    from loss.combine_loss import DeepSuperloss, FLPlusDice
    from models.HDenseFormer import HDenseFormer
    cfg = (2, 3, 16, (32, 32, 32), 8)
    sd = orc.det_model(*cfg)
    net = HDenseFormer(cfg[0], cfg[1], cfg[2], image_size=cfg[3], transformer_depth=cfg[4])
    net.load_state_dict(sd)
    net = net.to(DEV).eval()
    x = torch.from_numpy(detgen.det_input(2, cfg[0], cfg[3], tag="g11_g1"))
    onehot = torch.from_numpy(detgen.one_hot(detgen.det_labels(2, cfg[1], cfg[3], tag="g11_g1"), cfg[1]))
    outs = net(x.to(DEV))
    DeepSuperloss(criterion=FLPlusDice(None, 0))(outs, onehot.to(DEV)).backward()
    fused = {k: p.grad.detach().clone() for k, p in net.named_parameters()}
    for p in net.parameters():
        p.grad = None
    outs = net(x.to(DEV))
    _, dl = restated([o.detach().cpu() for o in outs], onehot, (1.0, 1.0, 2.0, "mean", 1.0, None, 0))
    torch.autograd.backward(list(outs), [d.float().to(DEV) for d in dl])
    torch.cuda.synchronize()
    total = sum(float(v.double().norm()) ** 2 for v in fused.values()) ** 0.5
    worst = ("", 0.0)
    for k, p in net.named_parameters():
        if float(p.grad.double().norm()) < 1e-6 * total:
            continue
        worst = max(worst, (k, rl2(fused[k], p.grad)), key=lambda kv: kv[1])
    print(f"  worst live tensor {worst[0]} rel-l2 {worst[1]:.2e}")
    assert worst[1] <= 1e-4


# ------------------------------------------------------------------------------------ (h) errors


def test_bad_inputs_raise():
    from hdf_rt import _lib
    from loss.combine_loss import DeepSuperloss
    from loss.cross_entropy import FocalLoss
    crit = DeepSuperloss(criterion=FocalLoss())
    t = torch.zeros(1, 2, 8, 8, 8)
    with pytest.raises(_lib.HdfError):                      # CPU tensors
        crit([torch.zeros(1, 2, 8, 8, 8)], t)
    with pytest.raises(_lib.HdfError):                      # mixed dtypes
        crit([torch.zeros(1, 2, 8, 8, 8, device=DEV), torch.zeros(1, 2, 4, 4, 4, device=DEV, dtype=torch.bfloat16)],
             t.to(DEV))
    with pytest.raises(_lib.HdfError):                      # n_cls = 9
        crit([torch.zeros(1, 9, 8, 8, 8, device=DEV)], torch.zeros(1, 9, 8, 8, 8, device=DEV))
    with pytest.raises(AssertionError):                     # shape mismatch
        crit([torch.zeros(1, 2, 8, 8, 4, device=DEV)], t.to(DEV))
