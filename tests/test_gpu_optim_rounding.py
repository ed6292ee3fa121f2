"""The optimizer kernels held to fp64, element by element: hdf_optim_step (Adam, AdamW, SGD) and hdf_adam_step on raw
buffers, one step from a prepared state with word 0 of step_state preset to k - 1, every element of p, s1 and s2 against
optim_ref.step64 within optim_ref.bound -- a first-order running error of the kernel's own fp32 operations, computed from
the reference alone, times K = 2 (tests/optim_ref.py says where K comes from; tests/test_optim_ref_cpu.py shows that
torch's fp32 step passes at half the bound and that a wrong decay, mask, group, bias correction, flag or scale does not
pass).  The gate of test_gpu_optim.py, 1e-5 of a tensor's maximum over 8 steps at lr 1e-3 and weight_decay 1e-4, sees none
of those.

optim_ref.CASES: steps 1, 2, 3, 5, 685 and 3000 (the counter restored to a large value); different lr and wd in the two
groups under a random mask; SGD with and without Nesterov and without momentum; grad_mul 0.37 with a loss scale of 3, a
scale of 1024, no scale; n = 1, 2, 3, 5, 1027, and one pass of the grid + 1201 (the grid-stride loop's second trip, then
the scalar tail); Adam with decay in the unmasked group only; hdf_adam_step beyond one pass of its grid, with and without
a mask.  Behind every buffer lie 64 guard elements that must come back bit for bit.  Then: SGD's first step does not read
the buffer it finds; a skipped step (*found_inf 1, inf, NaN, with a NaN behind grad_scale) leaves p, s1, s2 and the
counter bit for bit and the same call with found_inf cleared is step k; and the wrappers FlatSGD / FlatAdamW / FlatAdam
over the model's flat buffer, two steps with different lr per group and weight_decay 0.1, per element against step64
applied twice with the allowance of step 1 carried through step 2 -- which pins weight_decay_mask(), the order of the
groups and _rule_args against oracle.hdf_oracle.param_groups.

Each check prints one line "ROUNDING <case> <worst error / bound>" (pytest -s shows them)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import optim_ref as R  # noqa: E402
from hdf_rt._lib import check, lib, ptr, stream_ptr  # noqa: E402

DEV = "cuda:0"
FILL = {torch.float32: 7.0, torch.uint8: 0xA5, torch.int32: 0x5A5A5A5A}
CFG_TINY = (2, 3, 16, (32, 32, 32), 8)


def _case(name):
    return R.CASES[R.CASE_IDS.index(name)]


@functools.lru_cache(maxsize=2)
def _ref(name):
    case = _case(name)
    d = R.make(case)
    args = (case["rule"], d["p"], d["g"], d["s1"], d["s2"], d["mask"] != 0, case["step"], case["h"])
    return case, d, R.step64(*args), R.bound(*args)


def _guarded(t):
    buf = torch.full((t.numel() + R.GUARD,), FILL[t.dtype], dtype=t.dtype)
    buf[:t.numel()] = t
    return buf.to(DEV)


class Call:
    """the device buffers of one case, each followed by its guard, and the entry's call on them"""

    def __init__(self, case, d, s1=None):
        self.case, self.n = case, case["n"]
        h = case["h"]
        ctl = torch.zeros(8, dtype=torch.int32)
        ctl[0] = case["step"] - 1
        host = {"p": d["p"], "g": d["g"], "s1": d["s1"] if s1 is None else s1, "s2": d["s2"], "mask": d["mask"], "ctl": ctl,
                "scale": None if h["grad_scale"] is None else torch.tensor([h["grad_scale"]], dtype=torch.float32),
                "found_inf": torch.zeros(1, dtype=torch.float32)}
        self.buf = {k: _guarded(v) for k, v in host.items() if v is not None}
        self.size = {k: v.numel() for k, v in host.items() if v is not None}
        self.inputs = {k: self.buf[k].clone() for k in ("g", "mask")}

    def _ptr(self, key):
        return ptr(self.buf[key]) if key in self.buf else None

    def step(self, found_inf=False):
        case, h = self.case, self.case["h"]
        if case["entry"] == "adam":
            check(lib().hdf_adam_step(self._ptr("p"), self._ptr("g"), self._ptr("s1"), self._ptr("s2"),
                                      self._ptr("mask") if case["mask"] else None, self.n, h["lr"][0], h["b1"], h["b2"],
                                      h["eps"], h["wd"][0], case["step"], h["grad_mul"], stream_ptr()), "hdf_adam_step")
        else:
            check(lib().hdf_optim_step(case["rule"], self._ptr("p"), self._ptr("g"), self._ptr("s1"), self._ptr("s2"),
                                       self._ptr("mask"), self.n, h["lr"][0], h["lr"][1], h["wd"][0], h["wd"][1], h["b1"],
                                       h["b2"], h["eps"], h["nesterov"], h["grad_mul"], self._ptr("scale"),
                                       self._ptr("found_inf") if found_inf else None, self._ptr("ctl"), stream_ptr()),
                  "hdf_optim_step")

    def state(self):
        """(p, s1, s2) on the host, s2 None for SGD"""
        return tuple(self.buf[k][:self.n].cpu() if k in self.buf else None for k in ("p", "s1", "s2"))

    def counter(self):
        return int(self.buf["ctl"][0])

    def check_guards(self):
        for k, b in self.buf.items():
            guard = b[self.size[k]:].cpu()
            assert guard.numel() == R.GUARD and bool((guard == FILL[b.dtype]).all()), "%s: guard of %s written" % (
                self.case["name"], k)
        for k, b in self.inputs.items():
            assert torch.equal(self.buf[k], b), "%s: input %s written" % (self.case["name"], k)


@pytest.mark.parametrize("name", R.CASE_IDS)
def test_one_step_against_fp64(name):
    case, d, ref, allow = _ref(name)
    call = Call(case, d)
    call.step()
    R.held(name, call.state(), ref, allow)
    call.check_guards()
    if case["entry"] == "optim":
        assert call.counter() == case["step"]


@pytest.mark.parametrize("name", ["SGD.step1", "SGD.plain.step1"])
def test_sgd_first_step_does_not_read_the_buffer_it_finds(name):
    case, d, ref, allow = _ref(name)
    assert bool((d["s1"] != 0).all())
    a, b = Call(case, d), Call(case, d, s1=-7.0 * d["s1"])
    a.step()
    b.step()
    for x, y in zip(a.state()[:2], b.state()[:2]):
        assert torch.equal(x, y)
    R.held(name + ".other_buffer", b.state(), ref, allow)


def _bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("flag", [1.0, float("inf"), float("nan")], ids=["one", "inf", "nan"])
@pytest.mark.parametrize("rule", list(R.RULE_NAME.values()))
def test_skipped_step_touches_nothing_and_the_next_call_is_step_k(rule, flag):
    name = rule + ".gmul0.37_scale3"
    case, d, ref, allow = _ref(name)
    call = Call(case, d)
    before = [t.clone() for t in call.state() if t is not None]
    call.buf["found_inf"][0] = flag
    call.buf["scale"][0] = float("nan")                         # a skipped step must not use the scale it finds
    call.step(found_inf=True)
    for x, y in zip(before, [t for t in call.state() if t is not None]):
        assert torch.equal(_bits(x), _bits(y))
    assert call.counter() == case["step"] - 1
    call.check_guards()
    call.buf["found_inf"][0] = 0.0
    call.buf["scale"][0] = case["h"]["grad_scale"]
    call.step(found_inf=True)
    R.held("%s.after_skip_%s" % (name, flag), call.state(), ref, allow)
    assert call.counter() == case["step"]
    call.check_guards()


# ------------------------------------------------------------------------------------------------ the wrappers
def _wrapper_hyper(name):
    if name == "FlatSGD":
        return R.SGD, R.hyper(lr=(1e-2, 3e-3), wd=(0.1, 0.0), b1=0.9, nesterov=1)
    return (R.ADAMW if name == "FlatAdamW" else R.ADAM), R.hyper(lr=(1e-2, 3e-3), wd=(0.1, 0.0))


@pytest.mark.parametrize("name", ["FlatSGD", "FlatAdamW", "FlatAdam"])
def test_wrappers_two_steps_against_fp64(name):
    """the reference knows nothing of the flat layout: parameters in named_parameters() order, the group of each from
    oracle.hdf_oracle.param_groups, the constructors' defaults for everything but lr and weight_decay"""
    from hdf_rt import optim
    from models.HDenseFormer import HDenseFormer
    from oracle import hdf_oracle as orc
    in_ch, n_cls, nf, size, td = CFG_TINY
    sd = orc.det_model(*CFG_TINY)
    net = HDenseFormer(in_ch, n_cls, nf, image_size=size, transformer_depth=td)
    net.load_state_dict(sd)
    net = net.to(DEV)
    opt = getattr(optim, name)(net, lr=1e-2, weight_decay=0.1)
    opt.param_groups[1]["lr"] = 3e-3
    names = [k for k, _ in net.named_parameters()]
    decay, no_decay = orc.param_groups([(k, tuple(sd[k].shape)) for k in names])
    assert decay and no_decay and sorted(decay + no_decay) == sorted(names)
    dec = torch.cat([torch.full((sd[k].numel(),), k in decay, dtype=torch.bool) for k in names])
    rule, h = _wrapper_hyper(name)
    zero = torch.zeros(dec.numel(), dtype=torch.float64)
    p, s1, s2 = R.T(torch.cat([sd[k].flatten() for k in names]).double()), R.T(zero), None if rule == R.SGD else R.T(zero)
    for step in (1, 2):
        net.flat_grads()
        gen = torch.Generator().manual_seed(40 + step)
        grads = []
        for (k, q), view in zip(net.named_parameters(), net._grad_views):
            gr = torch.randn(q.shape, generator=gen) * 0.01
            view.copy_(gr.to(DEV))
            grads.append(gr.flatten())
        opt.step()
        p, s1, s2 = R.track(rule, p, R.T(torch.cat(grads).double()), s1, s2, dec, step, h)
    assert int(opt.step_counter) == 2
    got = torch.cat([q.detach().flatten().cpu() for _, q in net.named_parameters()])
    # per parameter tensor, so that a failure names it
    worst, at = 0.0, 0
    for k in names:
        sl = slice(at, at + sd[k].numel())
        r = R.ratio(got[sl], p.v[sl], R.K * p.e[sl])
        assert r <= 1.0, "%s: %s (%s group) at %.2f of the bound after two steps" % (
            name, k, "decay" if k in decay else "no-decay", r)
        worst, at = max(worst, r), sl.stop
    print("ROUNDING %s.two_steps %.3f" % (name, worst))
    # the state buffers lie over the flat buffer: each parameter's slice is where the parameter itself aliases it
    flat = net.flat_parameters()
    at = [(q.data_ptr() - flat.data_ptr()) // 4 for _, q in net.named_parameters()]
    assert all(0 <= a and a + sd[k].numel() <= flat.numel() for a, k in zip(at, names))
    state = [torch.cat([getattr(opt, n)[a: a + sd[k].numel()] for a, k in zip(at, names)]).cpu() for n in opt._state_names]
    R.held(name + ".two_steps.state", (got,) + tuple(state) + (None,) * (2 - len(state)),
           (p.v, s1.v, None if s2 is None else s2.v), (R.K * p.e, R.K * s1.e, None if s2 is None else R.K * s2.e))
