"""CPU-side checks of the optimizer surface (hdf_rt.optim): the flat optimizers are torch.optim.Optimizer subclasses over
the reference's two parameter groups, torch's schedulers and the project's PolyLR drive them, build_optimizer mirrors
trainer.py:_get_optimizer, and hdf_optim_step refuses bad arguments before it launches anything."""
import ctypes as C
import os

import pytest
import torch

from conftest import ROOT
from oracle import hdf_oracle as orc

OPTIMIZERS = ["FlatAdam", "FlatAdamW", "FlatSGD"]


def _net():
    from models.HDenseFormer import HDenseFormer_16
    return HDenseFormer_16(2, 3, (32, 32, 32), 8)


def _make(name, net, **kw):
    from hdf_rt import optim
    return getattr(optim, name)(net, **kw)


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


@pytest.mark.parametrize("name", OPTIMIZERS)
def test_flat_optimizers_are_torch_optimizers_over_the_reference_groups(name):
    net = _net()
    opt = _make(name, net, lr=1e-3, weight_decay=1e-4)
    assert isinstance(opt, torch.optim.Optimizer)
    decay, no_decay = orc.param_groups([(n, tuple(p.shape)) for n, p in net.named_parameters()])
    names = {id(p): n for n, p in net.named_parameters()}
    assert len(opt.param_groups) == 2
    got = [[names[id(p)] for p in g["params"]] for g in opt.param_groups]
    assert got[0] == decay and got[1] == no_decay
    assert sorted(got[0] + got[1]) == sorted(names.values()) and len(got[0]) + len(got[1]) == len(names)
    assert opt.param_groups[0]["weight_decay"] == 1e-4 and opt.param_groups[1]["weight_decay"] == 0.0
    assert opt.param_groups[0]["lr"] == opt.param_groups[1]["lr"] == 1e-3
    assert opt._step_supports_amp_scaling is True


@pytest.mark.parametrize("name", OPTIMIZERS)
def test_a_third_parameter_group_is_refused(name):
    opt = _make(name, _net())
    with pytest.raises(ValueError, match="two parameter groups"):
        opt.add_param_group({"params": [torch.nn.Parameter(torch.zeros(3))]})
    assert len(opt.param_groups) == 2


def _schedulers(opt):
    from hdf_rt.optim import PolyLR
    sch = torch.optim.lr_scheduler
    return {"MultiStepLR": (sch.MultiStepLR(opt, milestones=[2], gamma=0.1), ()),
            "CosineAnnealingLR": (sch.CosineAnnealingLR(opt, T_max=8), ()),
            "ReduceLROnPlateau": (sch.ReduceLROnPlateau(opt, patience=0, factor=0.5), (1.0,)),
            "PolyLR": (PolyLR(opt, max_epochs=8), ())}


@pytest.mark.parametrize("which", ["MultiStepLR", "CosineAnnealingLR", "ReduceLROnPlateau", "PolyLR"])
@pytest.mark.parametrize("name", OPTIMIZERS)
def test_schedulers_construct_and_move_lr_in_both_groups(name, which):
    opt = _make(name, _net(), lr=1e-3)
    sched, args = _schedulers(opt)[which]
    opt._opt_called = True      # no device here: the schedulers only warn when step() has not run before theirs
    for _ in range(4):          # (ReduceLROnPlateau: a metric that never improves)
        sched.step(*args)
    lrs = [g["lr"] for g in opt.param_groups]
    assert lrs[0] == lrs[1] and 0 < lrs[0] < 1e-3, (which, lrs)


@pytest.mark.parametrize("name", OPTIMIZERS)
def test_polylr_matches_the_closed_form(name):
    from hdf_rt.optim import PolyLR
    base_lr, max_epochs, ck_epoch, exponent = 3e-3, 6, 1, 0.9
    opt = _make(name, _net(), lr=base_lr)
    sched = PolyLR(opt, max_epochs, ck_epoch=ck_epoch, exponent=exponent)
    opt._opt_called = True
    want = None
    for epoch in range(max_epochs + 2 + 1):
        if epoch <= max_epochs:
            want = base_lr * (1 - (epoch - ck_epoch) / (max_epochs - ck_epoch)) ** exponent
        # epoch > max_epochs: frozen at the last value
        assert sched.last_epoch == epoch
        assert [g["lr"] for g in opt.param_groups] == [want, want], epoch
        assert sched.get_last_lr() == [want, want]
        sched.step()


def test_build_optimizer_mirrors_get_optimizer():
    from hdf_rt.optim import FlatAdam, FlatAdamW, FlatSGD, build_optimizer
    net = _net()
    for name in ("SGD", "sgd"):
        opt = build_optimizer(name, net, 2e-3, 3e-4, momentum=0.8)
        assert type(opt) is FlatSGD
        g0, g1 = opt.param_groups
        assert (g0["lr"], g0["momentum"], g0["nesterov"], g0["weight_decay"]) == (2e-3, 0.8, True, 3e-4)
        assert (g1["lr"], g1["momentum"], g1["nesterov"], g1["weight_decay"]) == (2e-3, 0.8, True, 0.0)
    assert build_optimizer("sgd", net, 2e-3, 3e-4).param_groups[0]["momentum"] == 0.9
    opt = build_optimizer("AdamW", net, 2e-3, 3e-4)
    assert type(opt) is FlatAdamW
    g0, g1 = opt.param_groups
    assert (g0["lr"], tuple(g0["betas"]), g0["eps"], g0["weight_decay"]) == (2e-3, (0.9, 0.999), 1e-8, 3e-4)
    assert g1["weight_decay"] == 0.0 and g1["lr"] == 2e-3
    opt = build_optimizer("Adam", net, 2e-3, 3e-4)
    assert type(opt) is FlatAdam
    g0, g1 = opt.param_groups
    ref = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))]).defaults      # torch's defaults, as the reference uses
    assert (g0["lr"], tuple(g0["betas"]), g0["eps"], g0["weight_decay"]) == (2e-3, tuple(ref["betas"]), ref["eps"], 3e-4)
    assert g1["weight_decay"] == 0.0
    with pytest.raises(ValueError):
        build_optimizer("rmsprop", net, 2e-3, 3e-4)


def test_optim_step_is_declared_and_refuses_bad_arguments(lib):
    """Every refusal is HDF_ERR_ARG (1) with a message: the argument checks come before any launch (a launch on this
    host, which has no device, would come back as HDF_ERR_HIP = 2)."""
    from hdf_rt import _lib
    hdr = open(os.path.join(ROOT, "include", "hdf.h")).read()
    assert "int hdf_optim_step(" in hdr and "hdf_optim_step" in _lib.EXPORTS and hasattr(lib, "hdf_optim_step")
    buf = (C.c_float * 68)()
    a = (C.addressof(buf) + 15) & ~15   # a 16-byte aligned host address: never dereferenced, every call stops at the checks
    p, g, s1, s2, mask, ctl = a, a + 64, a + 128, a + 192, a + 16, a + 32

    def call(rule=0, p=p, g=g, s1=s1, s2=s2, mask=mask, n=16, b1=0.9, b2=0.999, nesterov=0, ctl=ctl):
        return lib.hdf_optim_step(rule, p, g, s1, s2, mask, n, 1e-3, 1e-3, 1e-4, 0.0, b1, b2, 1e-8, nesterov, 1.0, None,
                                  None, ctl, None)

    bad = {"unknown rule": dict(rule=3), "negative rule": dict(rule=-1), "n < 0": dict(n=-1),
           "null params": dict(p=None), "null grads": dict(g=None), "null state": dict(s1=None),
           "null second moment": dict(s2=None), "null mask": dict(mask=None), "null step state": dict(ctl=None),
           "sgd momentum 1": dict(rule=2, b1=1.0, s2=None), "sgd momentum < 0": dict(rule=2, b1=-0.1, s2=None),
           "nesterov without momentum": dict(rule=2, b1=0.0, nesterov=1, s2=None),
           "beta1 1": dict(b1=1.0), "misaligned params": dict(p=a + 4)}
    for what, kw in bad.items():
        rc = call(**kw)
        assert rc == 1, (what, rc, lib.hdf_last_error())
        msg = lib.hdf_last_error()
        assert msg.startswith(b"optim_step:") and len(msg) > len(b"optim_step:"), (what, msg)
    # nothing to do is not an error, and launches nothing either
    assert call(n=0) == 0 and call(rule=2, n=0, s2=None) == 0
