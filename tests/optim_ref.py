"""The reference side of test_gpu_optim_rounding.py, CPU only: one step of Adam, AdamW or SGD in fp64 from arbitrary state
by the rules include/hdf.h states at hdf_optim_step (step64), a per-element allowance for the fp32 kernel computed from the
reference alone (bound), the same step with one thing wrong (MUTANTS), torch's own fp32 optimizers stepped once from the
same state (torch_step), and the cases both test files run (CASES, make).  tests/test_optim_ref_cpu.py shows that torch's
fp32 step passes the bound on every case and that every mutant fails it.

The operation.  Two groups chosen by the mask byte: lr / wd [0] where it is set, [1] elsewhere.  g' = g * grad_mul /
grad_scale.  Adam: g' += wd p;  m = b1 m + (1 - b1) g';  v = b2 v + (1 - b2) g'^2;  p -= (lr / bc1) m / (sqrt(v) / bc2s +
eps) with bc1 = 1 - b1^k, bc2s = sqrt(1 - b2^k).  AdamW: the same with p *= 1 - lr wd first and no wd p in g'.  SGD:
g' += wd p;  buf = g' at step 1 WHATEVER the buffer held, b1 buf + g' afterwards;  p -= lr (g' + b1 buf) with Nesterov,
lr buf without.  k is the 1-based number of this step.  Hyper-parameters are taken at the fp32 values the ABI carries
(hyper() rounds them: float(np.float32(x))), since that is the operation the kernel is asked for; the bias corrections
are formed from them in double and nothing is rounded.  torch forms its corrections from the Python doubles: for
betas = (0.9, 0.999) its sqrt(1 - b2^k) is 6.4e-6 (relative) away at small k (test_optim_ref_cpu.py holds the figure), so
torch_step hands torch the fp32-valued numbers as well.

The bound.  Values travel with a first-order running error (class T).  Every fp32 operation of adam_elem / optim_elem
(csrc/optim.h, optim.hip) adds U = 2^-24 of its result's magnitude, the one rounding of a correctly rounded operation; an
incoming error is scaled by the operation's derivative (product: |a| e_b + |b| e_a;  quotient: e_a / |b| + |q| e_b / |b|;
sqrt: e_v / (2 sqrt v)).  The constants a kernel rounds before it starts (1 - b, 1 - lr wd, bc1, bc2s, lr / bc1) count as
operations.  x / 1 is exact, so the division by the loss scale is charged only where a scale is given.  The allowance is
K times the running error of p, s1 and s2.  K = 2: torch's own fp32 step (another order of the same operations: lerp for
the first moment, no fma) measured against the unscaled (K = 1) running error on the cases below,
    worst |torch fp32 - step64| / running error:   Adam 0.984   AdamW 0.975   SGD 0.998   (hdf_adam_step's cases 0.982)
that is at most 0.499 of the bound (the last rounding of p alone reaches U |p| just above a power of two); test_optim_ref_cpu.py asserts <= 0.5 on every case.  A case that needed K above 4 would
mean a missing term.

Two steps (the wrappers): track() takes and returns T, so the error of step 1 goes through step 2 by the same rules."""
import math
import os

import numpy as np
import torch

ADAM, ADAMW, SGD = 0, 1, 2                      # HDF_OPTIM_* of include/hdf.h
RULE_NAME = {ADAM: "Adam", ADAMW: "AdamW", SGD: "SGD"}
U = 2.0 ** -24
K = 2.0
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hdf.h")
GUARD = 64                                      # elements behind every device buffer that must come back bit for bit
NVEC_PASS = 2048 * 256 * 4                      # elements one pass of optim_kernel's grid covers
NADAM_PASS = 4096 * 256                         # ... of adam_kernel's


def f32(x):
    return float(np.float32(x))


def hyper(lr=(1e-2, 3e-3), wd=(0.1, 0.02), b1=0.9, b2=0.999, eps=1e-8, nesterov=1, grad_mul=1.0, grad_scale=None):
    """the hyper-parameters of one call at the fp32 values the ABI carries.  lr / wd: (where the mask byte is set, the
    rest);  b1: beta1, or SGD's momentum;  grad_scale: the value behind the device pointer, None for a null pointer"""
    return {"lr": (f32(lr[0]), f32(lr[1])), "wd": (f32(wd[0]), f32(wd[1])), "b1": f32(b1), "b2": f32(b2), "eps": f32(eps),
            "nesterov": int(nesterov), "grad_mul": f32(grad_mul),
            "grad_scale": None if grad_scale is None else f32(grad_scale)}


# ------------------------------------------------------------------------------------ values with a running error
class T:
    """value and first-order running error, both fp64 (tensors, or floats for the constants)"""
    __slots__ = ("v", "e")

    def __init__(self, v, e=None):
        self.v = v
        self.e = e if e is not None else (torch.zeros_like(v) if torch.is_tensor(v) else 0.0)


def _abs(x):
    return x.abs() if torch.is_tensor(x) else abs(x)


def _rn(v, e):
    return T(v, e + U * _abs(v))


def _lift(x):
    return x if isinstance(x, T) else T(x)


def _mul(a, b):
    a, b = _lift(a), _lift(b)
    return _rn(a.v * b.v, _abs(a.v) * b.e + _abs(b.v) * a.e)


def _add(a, b):
    a, b = _lift(a), _lift(b)
    return _rn(a.v + b.v, a.e + b.e)


def _div(a, b):
    a, b = _lift(a), _lift(b)
    q = a.v / b.v
    return _rn(q, a.e / _abs(b.v) + _abs(q) * b.e / _abs(b.v))


def _sqrt(a):
    s = a.v.sqrt()
    return _rn(s, a.e / (2.0 * s.clamp_min(1e-300)))


def _fma(a, b, c):
    a, b, c = _lift(a), _lift(b), _lift(c)
    return _rn(a.v * b.v + c.v, _abs(a.v) * b.e + _abs(b.v) * a.e + c.e)


def _const(x):
    """a constant the kernel (or its host side) forms in higher precision and rounds to fp32 once"""
    return T(x, U * _abs(x))


# ------------------------------------------------------------------------------------ the step, right and wrong
MUTANTS = {
    # name: (rules, what is wrong)
    "decay_dropped": ((ADAM, ADAMW, SGD), "no weight decay at all"),
    "mask_inverted": ((ADAM, ADAMW, SGD), "the groups chosen by the inverted mask"),
    "lr_swapped": ((ADAM, ADAMW, SGD), "lr of the two groups swapped"),
    "wd_rest_ignored": ((ADAM, ADAMW, SGD), "wd of the unmasked group taken as 0"),
    "adamw_as_l2": ((ADAMW,), "AdamW's decay added to the gradient"),
    "adam_as_decoupled": ((ADAM,), "Adam's decay applied as p *= 1 - lr wd"),
    "bias_step_plus": ((ADAM, ADAMW), "bias corrections of step k + 1"),
    "bias_step_minus": ((ADAM, ADAMW), "bias corrections of step k - 1"),
    "bias_pow_rounded": ((ADAM, ADAMW), "b^k rounded to fp32 before 1 - b^k (the kernels before this file)"),
    "nesterov_ignored": ((SGD,), "the other branch of the Nesterov flag"),
    "grad_mul_ignored": ((ADAM, ADAMW, SGD), "grad_mul taken as 1"),
    "grad_scale_multiplied": ((ADAM, ADAMW, SGD), "g * grad_scale"),
    "sgd_first_step_adds": ((SGD,), "step 1 forms b1 buf + g' from the buffer it found"),
}


def applicable(mutant, rule, step, h, s1_nonzero=True):
    """whether `mutant` changes the result of this case at all (the conditions test_optim_ref_cpu.py states)"""
    if rule not in MUTANTS[mutant][0]:
        return False
    if mutant == "bias_step_minus":
        return step >= 2
    if mutant == "bias_pow_rounded":
        return step in (2, 3, 5)
    if mutant == "nesterov_ignored":
        return h["b1"] > 0.0
    if mutant == "grad_mul_ignored":
        return h["grad_mul"] != 1.0
    if mutant == "grad_scale_multiplied":
        return h["grad_scale"] not in (None, 1.0)
    if mutant == "sgd_first_step_adds":
        return step == 1 and h["b1"] > 0.0 and s1_nonzero
    if mutant in ("decay_dropped", "adamw_as_l2", "adam_as_decoupled"):
        return h["wd"] != (0.0, 0.0)
    if mutant == "wd_rest_ignored":
        return h["wd"][1] != 0.0
    if mutant == "lr_swapped":
        return h["lr"][0] != h["lr"][1]
    if mutant == "mask_inverted":
        return h["lr"][0] != h["lr"][1] or h["wd"][0] != h["wd"][1]
    return True


def groups_concerned(mutant, h):
    """the groups (1: mask set, 0: the rest) in EACH of which the mutant must leave an element of p beyond the bound; None
    for a mutant of something all elements share (the bias corrections, a flag, a scale): any element will do"""
    if mutant == "wd_rest_ignored":
        return (0,)
    if mutant in ("decay_dropped", "adamw_as_l2", "adam_as_decoupled"):
        return tuple(grp for grp, wd in ((1, h["wd"][0]), (0, h["wd"][1])) if wd != 0.0)
    if mutant in ("mask_inverted", "lr_swapped"):
        return (1, 0)
    return None


def _bias(b1, b2, step, rounded=False):
    if rounded:     # 1.f - (float)pow(b, k) and sqrt of THAT: what the kernels formed
        bc1 = f32(1.0 - f32(b1 ** step))
        return bc1, f32(math.sqrt(f32(1.0 - f32(b2 ** step))))
    return 1.0 - b1 ** step, math.sqrt(1.0 - b2 ** step)


def track(rule, p, g, s1, s2, dec, step, h, mutant=None):
    """one step on T values; dec: bool tensor (mask byte != 0).  Returns (p, s1, s2) as T (s2 None for SGD)."""
    assert mutant is None or mutant in MUTANTS
    dec = dec.bool()
    if mutant == "mask_inverted":
        dec = ~dec
    (lr0, lr1), (wd0, wd1) = h["lr"], h["wd"]
    if mutant == "lr_swapped":
        lr0, lr1 = lr1, lr0
    if mutant == "wd_rest_ignored":
        wd1 = 0.0
    if mutant == "decay_dropped":
        wd0 = wd1 = 0.0
    one = torch.ones_like(p.v)
    lr, wd = torch.where(dec, lr0 * one, lr1 * one), torch.where(dec, wd0 * one, wd1 * one)
    gmul = 1.0 if mutant == "grad_mul_ignored" else h["grad_mul"]
    b1, b2 = h["b1"], h["b2"]
    if h["grad_scale"] is not None:
        g = _mul(g, h["grad_scale"]) if mutant == "grad_scale_multiplied" else _div(g, h["grad_scale"])

    if rule == SGD:
        gi = _add(_mul(g, gmul), _mul(p, wd))
        first = step == 1 and mutant != "sgd_first_step_adds"
        buf = gi if first else _add(_mul(s1, b1), gi)
        nesterov = bool(h["nesterov"]) != (mutant == "nesterov_ignored")
        upd = _add(gi, _mul(buf, b1)) if nesterov else buf
        return _add(p, _mul(upd, -lr)), buf, None

    decoupled = (rule == ADAMW) != (mutant in ("adamw_as_l2", "adam_as_decoupled"))
    if decoupled:
        keep = 1.0 - lr * wd
        p = _mul(p, T(keep, torch.where(wd != 0.0, U * keep, 0.0 * keep)))
        gi = _fma(g, gmul, 0.0)
    else:
        gi = _fma(g, gmul, _mul(p, wd))
    m = _add(_mul(s1, b1), _mul(_const(1.0 - b1), gi))
    v = _add(_mul(s2, b2), _mul(_mul(_const(1.0 - b2), gi), gi))
    k = step + (mutant == "bias_step_plus") - (mutant == "bias_step_minus")
    bc1, bc2s = _bias(b1, b2, k, rounded=mutant == "bias_pow_rounded")
    denom = _add(_div(_sqrt(v), _const(bc2s)), h["eps"])
    ss = _div(lr, _const(bc1))
    q = _div(m, denom)
    return _rn(p.v - ss.v * q.v, p.e + _abs(ss.v) * q.e + _abs(q.v) * ss.e), m, v


def _lift64(x):
    return None if x is None else T(x.double())


def step64(rule, p, g, s1, s2, dec, step, h, mutant=None):
    """(p, s1, s2) after step number `step` in fp64 (s2 None for SGD)"""
    out = track(rule, _lift64(p), _lift64(g), _lift64(s1), _lift64(s2), dec, step, h, mutant)
    return tuple(None if t is None else t.v for t in out)


def bound(rule, p, g, s1, s2, dec, step, h, k=K):
    """the per-element allowance of (p, s1, s2) for an fp32 kernel that takes this step from exact fp32 inputs"""
    out = track(rule, _lift64(p), _lift64(g), _lift64(s1), _lift64(s2), dec, step, h)
    return tuple(None if t is None else k * t.e for t in out)


def ratio(got, ref, allow):
    """worst |got - ref| / allow over the elements (inf where an element is off and nothing is allowed)"""
    if got.numel() == 0:
        return 0.0
    err = (got.double() - ref).abs()
    r = torch.where(err > 0, err / allow.clamp_min(1e-300), torch.zeros_like(err))
    r = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), r)
    return float(r.max())


def held(case, got, ref, allow):
    """every element of every buffer within its allowance; prints the ROUNDING line; returns the worst ratio"""
    worst = 0.0
    for name, a, b, c in zip(("p", "s1", "s2"), got, ref, allow):
        if b is None:
            continue
        r = ratio(a, b, c)
        if not r <= 1.0:
            err = (a.double() - b).abs() / c.clamp_min(1e-300)
            i = int(torch.nan_to_num(err, nan=float("inf")).argmax())
            raise AssertionError("%s: %s[%d] = %.9g, fp64 reference %.9g, off by %.3e, allowed %.3e (%.2f of the bound)" % (
                case, name, i, float(a[i]), float(b[i]), abs(float(a[i]) - float(b[i])), float(c[i]), r))
        worst = max(worst, r)
    print("ROUNDING %s %.3f" % (case, worst))
    return worst


# ------------------------------------------------------------------------------------ the cases
def _case(name, rule, n, step, teeth=True, entry="optim", mask=True, zero_state=False, **hy):
    return {"name": name, "rule": rule, "n": n, "step": step, "teeth": teeth and n >= 1027, "entry": entry, "mask": mask,
            "zero_state": zero_state, "h": hyper(**hy)}


def _cases():
    out = []
    for rule, rn in RULE_NAME.items():
        for k in (1, 2, 3, 5, 685, 3000):
            # Adam's first step from the zero state a caller starts with; SGD's from a NON-zero buffer, which step 1 replaces
            out.append(_case("%s.step%d" % (rn, k), rule, 1027, k, zero_state=(k == 1 and rule != SGD)))
        out.append(_case("%s.gmul0.37_scale3" % rn, rule, 1027, 5, grad_mul=0.37, grad_scale=3.0))
        out.append(_case("%s.scale1024" % rn, rule, 1027, 5, grad_scale=1024.0))
        for n in (1, 2, 3, 5):
            out.append(_case("%s.n%d" % (rn, n), rule, n, 2))
        out.append(_case("%s.second_trip" % rn, rule, NVEC_PASS + 4 * 300 + 1, 2, teeth=False))     # (as step2, larger)
    for k in (1, 5):
        out.append(_case("SGD.plain.step%d" % k, SGD, 1027, k, nesterov=0))
        out.append(_case("SGD.momentum0.step%d" % k, SGD, 1027, k, b1=0.0, nesterov=0))
    out.append(_case("Adam.l2_rest_only", ADAM, 1027, 5, wd=(0.0, 0.02)))
    # hdf_adam_step: one lr, wd where the mask is set (nowhere without a mask), grad_scale MULTIPLIES (the ABI's grad_mul)
    out.append(_case("adam_step.nomask", ADAM, NADAM_PASS + 77, 2, entry="adam", mask=False, teeth=False,
                     lr=(1e-2, 1e-2), wd=(0.1, 0.0), grad_mul=0.37))
    out.append(_case("adam_step.mask", ADAM, NADAM_PASS + 77, 5, entry="adam", lr=(1e-2, 1e-2), wd=(0.1, 0.0),
                     grad_mul=0.37))
    return out


CASES = _cases()
CASE_IDS = [c["name"] for c in CASES]


def _loguniform(n, gen, lo=1e-3, hi=1e-1):
    mag = torch.exp(torch.rand(n, generator=gen, dtype=torch.float64) * math.log(hi / lo) + math.log(lo))
    return mag * (torch.randint(0, 2, (n,), generator=gen) * 2 - 1).double()


def make(case, seed=None):
    """the fp32 inputs of a case: p, g (as handed to the entry: times grad_scale / grad_mul), s1, s2 (None for SGD) and
    the mask bytes (all zero for the mask-less hdf_adam_step case).  |p| in [0.05, 1.05], |g * grad_mul / grad_scale| and
    the moment scale a log-uniform in [1e-3, 1e-1].  Adam's moments are those of a run that is k - 1 steps old whose
    gradient has shrunk: s1 = bc1(k - 1) a, s2 = bc2(k - 1) a^2 r with r log-uniform in [1/256, 1], so the update is up to
    16 lr and a wrong bias correction weighs against the rounding of p itself."""
    n, rule, k, h = case["n"], case["rule"], case["step"], case["h"]
    gen = torch.Generator().manual_seed(CASE_IDS.index(case["name"]) + 1000 if seed is None else seed)
    sign = (torch.randint(0, 2, (n,), generator=gen) * 2 - 1).double()
    p = (0.05 + torch.rand(n, generator=gen, dtype=torch.float64)) * sign
    g = _loguniform(n, gen) * (h["grad_scale"] or 1.0) / h["grad_mul"]
    a = _loguniform(n, gen)
    r = torch.exp(-math.log(256.0) * torch.rand(n, generator=gen, dtype=torch.float64))
    mask = (torch.rand(n, generator=gen) < 0.5).to(torch.uint8)
    # any non-zero byte selects the decay group, not bit 0 alone
    mask = mask * torch.tensor([1, 2, 0x80, 0xFF], dtype=torch.uint8)[torch.randint(0, 4, (n,), generator=gen)]
    if not case["mask"]:
        mask = torch.zeros(n, dtype=torch.uint8)
    if rule == SGD:
        s1, s2 = 3.0 * a, None
    else:
        bc1, bc2s = _bias(h["b1"], h["b2"], max(k - 1, 1))
        s1, s2 = bc1 * a, bc2s * bc2s * a * a * r
        if case["zero_state"]:
            s1, s2 = torch.zeros_like(s1), torch.zeros_like(s2)
    return {"p": p.float(), "g": g.float(), "s1": s1.float(), "s2": None if s2 is None else s2.float(), "mask": mask}


# ------------------------------------------------------------------------------------ torch's own fp32 step
def torch_step(case, d):
    """torch.optim.{Adam, AdamW, SGD}(foreach=False) in fp32, stepped once from the state of `d` seeded into
    optimizer.state, with the fp32-valued hyper-parameters of the case; the gradient it is given is (g / grad_scale) *
    grad_mul formed in fp32.  Returns (p, s1, s2) scattered back to the flat order; s1 is None where torch keeps no buffer
    (SGD without momentum)."""
    rule, k, h = case["rule"], case["step"], case["h"]
    g = d["g"].clone()
    if h["grad_scale"] is not None:
        g = g / torch.tensor(h["grad_scale"], dtype=torch.float32)
    g = g * torch.tensor(h["grad_mul"], dtype=torch.float32)
    sel = [d["mask"] != 0, d["mask"] == 0]
    params, groups = [], []
    for grp, idx in enumerate(sel):
        q = torch.nn.Parameter(d["p"][idx].clone())
        q.grad = g[idx].clone()
        params.append(q)
        if q.numel():
            groups.append({"params": [q], "lr": h["lr"][grp], "weight_decay": h["wd"][grp]})
    if rule == SGD:
        opt = torch.optim.SGD(groups, lr=1.0, momentum=h["b1"], nesterov=bool(h["nesterov"]), foreach=False)
    else:
        cls = torch.optim.Adam if rule == ADAM else torch.optim.AdamW
        opt = cls(groups, lr=1.0, betas=(h["b1"], h["b2"]), eps=h["eps"], foreach=False)
    for q, idx in zip(params, sel):
        if not q.numel():
            continue
        if rule == SGD:
            if k > 1 and h["b1"] > 0.0:
                opt.state[q]["momentum_buffer"] = d["s1"][idx].clone()
        else:
            opt.state[q].update(step=torch.tensor(float(k - 1)), exp_avg=d["s1"][idx].clone(),
                                exp_avg_sq=d["s2"][idx].clone())
    opt.step()
    out = []
    for key in ("p", "momentum_buffer" if rule == SGD else "exp_avg", "exp_avg_sq"):
        if key == "exp_avg_sq" and rule == SGD:
            out.append(None)
            continue
        if key == "momentum_buffer" and h["b1"] == 0.0:
            out.append(None)
            continue
        flat = torch.empty_like(d["p"])
        for q, idx in zip(params, sel):
            if q.numel():
                flat[idx] = q.detach() if key == "p" else opt.state[q][key]
        out.append(flat)
    return tuple(out)
