"""GPU checks of the flat optimizers (hdf_rt.optim.FlatAdam / FlatAdamW / FlatSGD -> hdf_optim_step): parity with torch's
own fp32 optimizers under a scheduler, bit-identity of the Adam rule with hdf_adam_step, the loss-scaling protocol
(device grad_scale / found_inf, skipped steps do not advance the bias correction), torch.amp.GradScaler without a host
synchronisation, and the state_dict round trip.

The parity gate, 1e-5 on the worst per-tensor max|a-b| / max|b|, is the project's Adam gate
(test_gpu_model.py::test_flat_adam_matches_torch_adam).  torch's fp32 optimizers against their own fp64 run on the same
inputs over 8 steps differ by 3.2e-7 (SGD), 5.6e-7 (AdamW) and 3.1e-7 (Adam): the gate leaves about 17x over the
reference's own rounding.  What it can see is a step that is grossly wrong (a missing update, a wrong sign, the bias
correction of another step, Adam's L2 decay gone: 1.2e-5).  What it cannot: at lr 1e-3 and weight_decay 1e-4 a dropped or
inverted weight decay moves the gated number by 1.6e-6 at the most, and the two groups share one lr, so a swapped group is
no change at all.  The arithmetic itself -- every element, both groups with their own lr and wd, grad_mul, loss scales,
every step count and length -- is held to fp64 in tests/test_gpu_optim_rounding.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import detgen  # noqa: E402
from oracle import hdf_oracle as orc  # noqa: E402

DEV = "cuda:0"
CFG_TINY = (2, 3, 16, (32, 32, 32), 8)
GATE = 1e-5
OPTIMIZERS = ["FlatSGD", "FlatAdamW", "FlatAdam"]


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def _build(cfg, dtype=None, sd=None):
    from models.HDenseFormer import HDenseFormer
    in_ch, n_cls, nf, size, td = cfg
    net = HDenseFormer(in_ch, n_cls, nf, image_size=size, transformer_depth=td)
    sd = orc.det_model(*cfg) if sd is None else sd
    net.load_state_dict(sd)
    net = net.to(DEV)
    net.compute_dtype = dtype
    return net, sd


def _data(cfg, batch, tag):
    in_ch, n_cls, nf, size, td = cfg
    x = torch.from_numpy(detgen.det_input(batch, in_ch, size, tag=tag))
    onehot = torch.from_numpy(detgen.one_hot(detgen.det_labels(batch, n_cls, size, tag=tag), n_cls))
    return x, onehot


def _make(name, net, **kw):
    from hdf_rt import optim
    return getattr(optim, name)(net, **kw)


def _torch_optimizer(name, groups):
    if name == "FlatSGD":
        return torch.optim.SGD(groups, momentum=0.9, nesterov=True, lr=1e-3, weight_decay=1e-4)
    if name == "FlatAdamW":
        return torch.optim.AdamW(groups, eps=1e-8, betas=(0.9, 0.999), lr=1e-3, weight_decay=1e-4)
    return torch.optim.Adam(groups, lr=1e-3, weight_decay=1e-4)


def _seed_grads(net, step, scale=1.0):
    """seeded 0.01*randn gradients into the flat gradient views; returns them by name (CPU, unscaled)"""
    net.flat_grads()
    g = torch.Generator().manual_seed(step)
    out = {}
    for (name, p), v in zip(net.named_parameters(), net._grad_views):
        gr = torch.randn(p.shape, generator=g) * 0.01
        v.copy_((gr * scale).to(DEV))
        out[name] = gr
    return out


def _snapshot(net, opt):
    counter = opt.step_counter.clone()          # (allocates the state of an optimizer that has not stepped yet)
    return [net.flat_parameters().clone(), counter] + [getattr(opt, n).clone() for n in opt._state_names]


@pytest.mark.parametrize("name", OPTIMIZERS)
def test_flat_optimizers_match_torch_under_a_scheduler(name):
    net, sd = _build(CFG_TINY)
    ref = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    decay, no_decay = orc.param_groups([(k, tuple(v.shape)) for k, v in ref.items()])
    topt = _torch_optimizer(name, [{"params": [ref[k] for k in decay]},
                                   {"params": [ref[k] for k in no_decay], "weight_decay": 0.0}])
    opt = _make(name, net, lr=1e-3, weight_decay=1e-4)
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[4], gamma=0.1)
    tsched = torch.optim.lr_scheduler.MultiStepLR(topt, milestones=[4], gamma=0.1)
    for step in range(8):
        for k, gr in _seed_grads(net, step).items():
            ref[k].grad = gr
        opt.step()
        topt.step()
        sched.step()
        tsched.step()
    assert [g["lr"] for g in opt.param_groups] == [g["lr"] for g in topt.param_groups]
    assert opt.param_groups[0]["lr"] == pytest.approx(1e-4)
    worst = max(_rel(p.detach(), ref[k].detach()) for k, p in net.named_parameters())
    print(f"  {name} vs torch, 8 steps, MultiStepLR: worst rel {worst:.3e}")
    assert worst < GATE
    assert int(opt.step_counter) == 8


def test_flat_adam_is_bit_identical_to_hdf_adam_step():
    from hdf_rt._lib import check, lib, ptr, stream_ptr
    net, _ = _build(CFG_TINY)
    opt = _make("FlatAdam", net, lr=1e-3, weight_decay=1e-4)
    flat = net.flat_parameters()
    start = flat.clone()
    p2, m2, v2 = flat.clone(), torch.zeros_like(flat), torch.zeros_like(flat)
    mask = net.weight_decay_mask()
    for step in range(3):
        _seed_grads(net, step)
        g = net.flat_grads()
        check(lib().hdf_adam_step(ptr(p2), ptr(g), ptr(m2), ptr(v2), ptr(mask), p2.numel(), 1e-3, 0.9, 0.999, 1e-8,
                                  1e-4, step + 1, 1.0, stream_ptr()), "hdf_adam_step")
        opt.step()
        assert net.flat_parameters() is flat
        assert torch.equal(flat, p2), f"parameters differ at step {step + 1}"
        assert torch.equal(opt.exp_avg, m2) and torch.equal(opt.exp_avg_sq, v2), f"moments differ at step {step + 1}"
    assert not torch.equal(flat, start)


@pytest.mark.parametrize("rule", [0, 1, 2], ids=["Adam", "AdamW", "SGD"])
def test_tail_of_a_raw_buffer_whose_length_is_not_a_multiple_of_four(rule):
    """hdf_optim_step takes any n: the last n % 4 elements go through the scalar tail.  n = 4k + 3 on raw buffers against
    the same call over n + 1 (a multiple of four, so all of it takes the 16-byte loop): the first n elements must be
    bit-identical, and the element behind the end of the short call must not be touched.  Two steps, so SGD's first-step
    initialisation and its running form are both seen."""
    from hdf_rt._lib import check, lib, ptr, stream_ptr
    n = 4 * 70001 + 3                                   # more than one workgroup of vectors, then a tail of three
    gen = torch.Generator().manual_seed(3)
    p0 = torch.randn(n + 1, generator=gen).to(DEV)
    mask = (torch.rand(n + 1, generator=gen) < 0.5).to(torch.uint8).to(DEV)
    sentinel = float(p0[n])

    def run(count):
        p, s1, s2 = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
        ctl = torch.zeros(8, dtype=torch.int32, device=DEV)
        for step in range(2):
            g = (torch.randn(n + 1, generator=torch.Generator().manual_seed(10 + step)) * 0.01).to(DEV)
            check(lib().hdf_optim_step(rule, ptr(p), ptr(g), ptr(s1), None if rule == 2 else ptr(s2), ptr(mask), count,
                                       1e-3, 2e-3, 1e-2, 0.0, 0.9, 0.999, 1e-8, int(rule == 2), 1.0, None, None,
                                       ptr(ctl), stream_ptr()), "hdf_optim_step")
        assert int(ctl[0]) == 2
        return p, s1, s2

    short, full = run(n), run(n + 1)
    for a, b in zip(short, full):
        assert torch.equal(a[:n], b[:n])
    assert not torch.equal(short[0][n - 3:n], p0[n - 3:n])          # the tail did move
    assert float(short[0][n]) == sentinel and float(short[1][n]) == 0.0 and float(short[2][n]) == 0.0
    assert float(full[0][n]) != sentinel


@pytest.mark.parametrize("name", OPTIMIZERS)
def test_loss_scaling_protocol_without_a_scaler(name):
    net, sd = _build(CFG_TINY)
    opt = _make(name, net, lr=1e-3, weight_decay=1e-4)
    net2, _ = _build(CFG_TINY)
    opt2 = _make(name, net2, lr=1e-3, weight_decay=1e-4)
    # found_inf set: nothing moves, the counter included
    _seed_grads(net, 0, scale=256.0)
    before = _snapshot(net, opt)
    opt.grad_scale = torch.tensor(256.0, device=DEV)
    opt.found_inf = torch.tensor(1.0, device=DEV)
    opt.step()
    for a, b in zip(before, _snapshot(net, opt)):
        assert torch.equal(a, b)
    assert int(opt.step_counter) == 0
    # found_inf clear, gradients 256 times too large: the unscaled step of the copy
    opt.found_inf = torch.tensor(0.0, device=DEV)
    opt.step()
    _seed_grads(net2, 0)
    opt2.step()
    worst = max(_rel(p.detach(), q.detach()) for p, q in zip(net.parameters(), net2.parameters()))
    print(f"  {name} scaled by 256 vs unscaled: worst rel {worst:.3e}")
    assert worst < GATE
    assert not torch.equal(before[0], net.flat_parameters())
    assert int(opt.step_counter) == 1 and int(opt2.step_counter) == 1
    # the skipped call did not count: the step above matched the copy's step 1, and the next one matches its step 2
    # (test_skipped_step_keeps_the_bias_correction_of_step_one pins the correction itself)
    del opt.grad_scale, opt.found_inf
    _seed_grads(net, 1)
    _seed_grads(net2, 1)
    opt.step()
    opt2.step()
    worst = max(_rel(p.detach(), q.detach()) for p, q in zip(net.parameters(), net2.parameters()))
    assert worst < GATE
    assert int(opt.step_counter) == 2 and opt.step_count == 3


def test_skipped_step_keeps_the_bias_correction_of_step_one():
    """Without weight decay Adam's first update is lr * sign(g) (to eps / |g|): m / bc1 = g and sqrt(v / bc2) = |g|.
    With the corrections of step 2 it would be (0.1 / 0.19) * sqrt(0.001999 / 0.001) = 0.744 of that.  One skipped call,
    then one taken: the update must be step 1's."""
    net, _ = _build(CFG_TINY)
    opt = _make("FlatAdam", net, lr=1e-3, weight_decay=0.0)
    _seed_grads(net, 0)
    before = net.flat_parameters().clone()
    opt.found_inf = torch.tensor(1.0, device=DEV)
    opt.step()
    opt.found_inf = torch.tensor(0.0, device=DEV)
    opt.step()
    g = net.flat_grads()
    big = g.abs() > 1e-4                                  # where eps = 1e-8 is below fp32 rounding of the ratio
    upd = (before - net.flat_parameters())[big]
    want = 1e-3 * torch.sign(g[big])
    err = float((upd - want).abs().max() / 1e-3)
    print(f"  first taken update vs lr*sign(g): {err:.3e}")
    assert err < 1e-3                                     # step 2's corrections would be off by 0.26


def _amp_run(name, init_scale):
    from loss.combine_loss import CEPlusDice, DeepSuperloss
    cfg, batch, tag = CFG_TINY, 2, "g1_tiny_eval"
    net, _ = _build(cfg, "fp16")
    net.train()
    x, onehot = _data(cfg, batch, tag)
    x, onehot = x.to(DEV), onehot.to(DEV)
    crit = DeepSuperloss(criterion=CEPlusDice(weight=None, ignore_index=0))
    opt = _make(name, net)
    scaler = torch.amp.GradScaler("cuda", init_scale=init_scale)
    return net, crit, opt, scaler, x, onehot


def _scaler_step_without_sync(scaler, opt):
    """scaler.step + scaler.update under torch's sync debug mode "error": any host synchronisation raises"""
    torch.cuda.synchronize()
    try:
        torch.cuda.set_sync_debug_mode("error")
    except Exception as e:      # only a torch build without the mode may go unchecked
        print(f"  torch.cuda.set_sync_debug_mode rejected ({e!r}): host-sync assertion not made")
        scaler.step(opt)
        scaler.update()
        return
    try:
        scaler.step(opt)
        scaler.update()
    finally:
        torch.cuda.set_sync_debug_mode("default")


@pytest.mark.parametrize("name", OPTIMIZERS)
def test_fp16_training_under_gradscaler_without_host_sync(name):
    net, crit, opt, scaler, x, onehot = _amp_run(name, 256.0)
    losses = []
    for _ in range(4):
        opt.zero_grad()
        loss = crit(net(x), onehot)
        scaler.scale(loss).backward()
        _scaler_step_without_sync(scaler, opt)
        losses.append(loss.item())
    print(f"  {name} fp16 losses", losses)
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]
    assert int(opt.step_counter) == 4 and scaler.get_scale() == 256.0


@pytest.mark.parametrize("name", OPTIMIZERS)
def test_gradscaler_overflow_skips_the_step_and_halves_the_scale(name):
    net, crit, opt, scaler, x, onehot = _amp_run(name, 2.0 ** 40)
    opt.zero_grad()
    loss = crit(net(x), onehot)
    scaler.scale(loss).backward()
    before = _snapshot(net, opt)
    _scaler_step_without_sync(scaler, opt)
    for a, b in zip(before, _snapshot(net, opt)):
        assert torch.equal(a, b)
    assert scaler.get_scale() == 2.0 ** 39
    assert int(opt.step_counter) == 0


@pytest.mark.parametrize("name", OPTIMIZERS)
def test_state_dict_round_trip_continues_the_run_exactly(name):
    def run(net, opt, steps):
        for step in steps:
            _seed_grads(net, step)
            opt.step()

    net, _ = _build(CFG_TINY)
    opt = _make(name, net, lr=1e-3, weight_decay=1e-4)
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[2], gamma=0.5)
    for step in range(6):
        run(net, opt, [step])
        sched.step()
    straight = net.flat_parameters().clone()

    net1, _ = _build(CFG_TINY)
    opt1 = _make(name, net1, lr=1e-3, weight_decay=1e-4)
    sched1 = torch.optim.lr_scheduler.MultiStepLR(opt1, milestones=[2], gamma=0.5)
    for step in range(3):
        run(net1, opt1, [step])
        sched1.step()
    saved = {k: v.detach().cpu().clone() for k, v in net1.state_dict().items()}
    osd, ssd = opt1.state_dict(), sched1.state_dict()
    assert int(osd["state"]["step"]) == 3 and osd["param_groups"][0]["lr"] == 5e-4
    assert all("params" not in g for g in osd["param_groups"])

    net2, _ = _build(CFG_TINY, sd=saved)
    opt2 = _make(name, net2)                    # default hyper-parameters: the saved ones must come from the state
    opt2.load_state_dict(osd)
    sched2 = torch.optim.lr_scheduler.MultiStepLR(opt2, milestones=[2], gamma=0.5)
    sched2.load_state_dict(ssd)
    assert opt2.param_groups[0]["weight_decay"] == 1e-4 and opt2.param_groups[1]["weight_decay"] == 0.0
    for step in range(3, 6):
        run(net2, opt2, [step])
        sched2.step()
    assert torch.equal(net2.flat_parameters(), straight)
    assert int(opt2.step_counter) == 6
