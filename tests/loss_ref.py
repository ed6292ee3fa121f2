"""CPU side of tests/test_gpu_loss_rounding.py and tests/test_loss_check_cpu.py: the seeded cases, the references of the
fused losses (oracle/hdf_oracle.py and tests/test_focal_loss_cpu.py, run with autograd in fp64 and in fp32) and the
closed-form logit gradient that lets the softmax be swapped for the one the kernels' fast intrinsics compute.  Nothing in
here touches a GPU or the kernels' output: every allowance below is a property of the reference alone."""
import functools
import math

import torch

from hdf_rt._lib import BF16, F16, F32
from hip_util import TDT, rnd, signed_rounding_bias
from oracle import hdf_oracle as orc

NAME = {F32: "f32", BF16: "bf16", F16: "f16"}
SMOOTH = 1e-5
CLASS_WEIGHT = [0.2, 1.0, 2.0, 0.5, 1.5, 0.7, 1.3, 0.9]

# name: (scale-0 shape, N, C, scales, options).  mul: logits scale; absent: class C-1 never in the target, class 1 never
# the argmax; unaligned: the GPU test hands logits and target over as views one element off 16 bytes
CASES = {
    "cap_vec4": ((72, 128, 120), 2, 4, 4, {}),
    "cap_vec1": ((64, 64, 66), 1, 6, 2, {}),
    "cap_2d": ((514, 514), 1, 2, 2, {}),
    "cap_unaligned": ((64, 64, 68), 1, 3, 1, dict(unaligned=1)),
    "small_odd": ((8, 16, 24), 3, 3, 4, {}),
    "c2": ((8, 8, 16), 1, 2, 2, {}),
    "c8": ((8, 8, 16), 1, 8, 2, {}),
    "absent": ((16, 16, 16), 2, 4, 4, dict(absent=1)),
    "saturated": ((8, 16, 16), 2, 4, 2, dict(mul=30.0)),
    "focal_vec4": ((72, 128, 120), 2, 2, 4, {}),      # cap_vec4 with the two classes of the focal losses
}
SEED = {k: 1000 + 17 * i for i, k in enumerate(CASES)}

# (w_ce, w_dice, class weight given, Dice ignore_index)
DEFAULT = (1.0, 1.0, False, 0)
WEIGHTED = (1.0, 1.0, True, 0)
FORMS = [(wc, wd, cw, ig) for (wc, wd) in ((1.0, 1.0), (0.0, 1.0), (1.0, 0.0)) for cw in (False, True) for ig in (0, None)]


def form_name(form):
    return "ce%g_dice%g_%s_ign%s" % (form[0], form[1], "w" if form[2] else "now", form[3])


def form_weight(form, c, dt=torch.float64):
    return torch.tensor(CLASS_WEIGHT[:c], dtype=dt) if form[2] else None


@functools.lru_cache(maxsize=2)
def inputs(case, dtype):
    """(logits per scale, storage-rounded, as fp32 CPU tensors; one-hot target fp32)"""
    shape, n, c, scales, o = CASES[case]
    gen = torch.Generator().manual_seed(SEED[case])
    lab = torch.randint(0, c - 1 if o.get("absent") else c, (n,) + shape, generator=gen)
    onehot = torch.nn.functional.one_hot(lab, c).movedim(-1, 1).float().contiguous()
    outs = []
    for i in range(scales):
        x = torch.randn((n, c) + tuple(d >> i for d in shape), generator=gen) * o.get("mul", 1.0)
        if o.get("absent"):
            x[:, 1] -= 12.0
        outs.append(rnd(x, dtype))
    return outs, onehot


def subsample(onehot, i):
    s = 1 << i
    return onehot[(slice(None), slice(None)) + (slice(None, None, s),) * (onehot.dim() - 2)]


# ------------------------------------------------------------------------------------------------ autograd references
def reference(outs, onehot, form, dt, gout=1.0):
    """DeepSuperloss(w_ce * CrossentropyLoss(weight) + w_dice * DiceLoss(weight, ignore_index)) of the oracle in dtype dt
    with autograd -> (loss as a Python float, [d (gout * loss) / d out_i])"""
    w_ce, w_dice, _, ign = form
    w = form_weight(form, onehot.shape[1], dt)
    ins = [o.to(dt, copy=True).requires_grad_(True) for o in outs]
    t = onehot.to(dt)
    if (w_ce, w_dice) == (1.0, 1.0):
        total = orc.deep_super_loss(ins, t, weight=w, ignore_index=ign)
    else:
        total = 0.0
        for i, o in enumerate(ins):
            sub = subsample(t, i)
            if w_ce:
                total = total + orc.ce_term(o, sub, w) * (w_ce / (2 ** i))
            if w_dice:
                total = total + orc.dice_term(o, sub, w, ign, SMOOTH) * (w_dice / (2 ** i))
    (total * gout).backward()
    return float(total.detach().double()), [x.grad for x in ins]


def restated_in(outs, target, spec, dt, softmax32=None):
    """tests/test_focal_loss_cpu.py `restated` with the arithmetic after the fp32 softmax in dtype dt (float64: `restated`
    itself, which tests/test_loss_check_cpu.py asserts) and, optionally, another fp32 softmax for the focal term"""
    from test_focal_loss_cpu import dice_loss, focal_dp, focal_map
    w_focal, alpha, gamma, red, w_dice, weight, ignore = spec
    t0 = torch.as_tensor(target).to(dt)
    total, grads = 0.0, []
    for i, o in enumerate(outs):
        t = subsample(t0, i)
        z = torch.as_tensor(o).detach().to(dt, copy=True).requires_grad_(True)
        p = torch.softmax(z, 1)
        pd = (softmax32(z.detach().float()) if softmax32 else torch.softmax(z.detach().float(), 1)).to(dt)
        den = float(pd.numel()) if red == "mean" else 1.0
        lf = focal_map(pd, t, alpha, gamma).sum() / den
        gp = focal_dp(pd, t, alpha, gamma) / den
        w = 1.0 / (1 << i)
        gz = w * w_focal * pd * (gp - (gp * pd).sum(1, keepdim=True))
        if w_dice:
            ld = dice_loss(p, t, weight, ignore)
            (w * w_dice * ld).backward()
            gz = gz + z.grad
            total += w * w_dice * float(ld.detach())
        total += w * w_focal * float(lf)
        grads.append(gz)
    return total, grads


# ------------------------------------------------------------------------------------------ the softmax, formed two ways
LOG2E32 = torch.tensor(math.log2(math.e), dtype=torch.float32)
LN2_32 = torch.tensor(math.log(2.0), dtype=torch.float32)


def softmax_a(x):
    """(A) fp64: p and logsumexp of the storage-rounded logits"""
    x = x.double()
    return torch.softmax(x, 1), torch.logsumexp(x, 1, keepdim=True)


def softmax_b(x):
    """(B) what the kernels' fast intrinsics compute, emulated in fp32: exp(d) as exp2(fl(d * log2 e)), the class sum taken
    class after class, p = e * (1 / se), log(se) as ln2 * log2(se).  Returned in fp64."""
    x = x.float()
    mx = x.max(1, keepdim=True).values
    e = torch.exp2((x - mx) * LOG2E32)
    se = torch.zeros_like(mx)
    for c in range(x.shape[1]):
        se = se + e[:, c:c + 1]
    p = e * (1.0 / se)
    lse = mx + LN2_32 * torch.log2(se)
    return p.double(), lse.double()


def closed_form(x, t, p, lse, form, i, gout=1.0, sums_of=None):
    """loss term and logit gradient of scale i in fp64, written out: with kce the CE coefficient of the voxel and G the
    Dice gradient with respect to p, d loss / d logit_c = kce (p_c - onehot_c) + p_c (G_c - <G, p>).  x: logits, t: the
    one-hot target on this scale's grid, (p, lse): the softmax in either form; sums_of: another target for the Dice sums and the CE denominator (a defect planted
    in the backward pass alone leaves those of the forward pass as they were).  -> (2^-i * term, gradient of gout * it)"""
    w_ce, w_dice, _, ign = form
    x, t, p, lse = x.double(), t.double(), p.double(), lse.double()
    n, c = x.shape[:2]
    bc = (1, c) + (1,) * (x.dim() - 2)
    w = form_weight(form, c)
    wc = w if w is not None else torch.ones(c, dtype=torch.float64)
    sw = 1.0 / (1 << i)
    ts = t if sums_of is None else sums_of.double()
    tc = t.argmax(1, keepdim=True)
    oh = torch.zeros_like(t).scatter_(1, tc, 1.0)
    wv = wc[tc]                                                   # [n, 1, ...]
    wsum = wc[ts.argmax(1, keepdim=True)].sum() if w is not None else float(tc.numel())
    ce = (wv * (lse - x.gather(1, tc))).sum() / wsum
    kce = w_ce * gout * sw * wv / wsum
    keep = torch.tensor([k != ign for k in range(c)], dtype=torch.float64)
    cd = c - 1 if ign is not None else c
    inter = (p * ts).flatten(2).sum(2)
    union = (p + ts).flatten(2).sum(2)
    dice = ((wc * keep) * (1.0 - (2.0 * inter + SMOOTH) / (union + SMOOTH)).mean(0)).sum() / cd
    a = (wc * keep * 2.0 / (union + SMOOTH)).view((n, c) + bc[2:])
    b = (wc * keep * (2.0 * inter + SMOOTH) / (union + SMOOTH) ** 2).view((n, c) + bc[2:])
    g = -(w_dice * gout * sw / (cd * n)) * (a * t - b)
    grad = kce * (p - oh) + p * (g - (g * p).sum(1, keepdim=True))
    return float((sw * (w_ce * ce + w_dice * dice)).detach()), grad


@functools.lru_cache(maxsize=1)
def softmaxes(case, dtype):
    outs, _ = inputs(case, dtype)
    return [softmax_a(o) for o in outs], [softmax_b(o) for o in outs]


def closed_both(case, dtype, form, gout=1.0):
    """((loss A, [grad A per scale]), (loss B, [grad B per scale]))"""
    outs, onehot = inputs(case, dtype)
    res = []
    for sm in softmaxes(case, dtype):
        loss, grads = 0.0, []
        for i, (o, (p, lse)) in enumerate(zip(outs, sm)):
            li, gi = closed_form(o, subsample(onehot, i), p, lse, form, i, gout)
            loss += li
            grads.append(gi)
        res.append((loss, grads))
    return res


# ------------------------------------------------------------------------------------------------ what a test holds to
def held_to(case, dtype, form, gout=1.0):
    """dict(loss64, grads64, acc=[per scale], loss_tol): the fp64 reference of one case and the allowances of the issue --
    acc_i = 4 max|grad(fp32 reference) - grad(fp64 reference)| + max|grad(A) - grad(B)|;
    loss_tol = 4 |loss(fp32 reference) - loss64| + |loss(A) - loss(B)| + 2^-24 |loss64|"""
    outs, onehot = inputs(case, dtype)
    l64, g64 = reference(outs, onehot, form, torch.float64, gout)
    l32, g32 = reference(outs, onehot, form, torch.float32, gout)
    (la, ga), (lb, gb) = closed_both(case, dtype, form, gout)
    acc = [4.0 * float((a.double() - b).abs().max()) + float((c - d).abs().max()) for a, b, c, d in zip(g32, g64, ga, gb)]
    return dict(loss64=l64, grads64=g64, acc=acc, loss_tol=4.0 * abs(l32 - l64) + abs(la - lb) + 2.0 ** -24 * abs(l64),
                closed=(la, ga))


def focal_spec(kind, c):
    """FocalLoss(0.25, 2, 'sum') / FLPlusDice(weight, 0) as the spec of `restated`"""
    if kind == "focal":
        return (1.0, 0.25, 2.0, "sum", 0.0, None, 0)
    return (1.0, 1.0, 2.0, "mean", 1.0, CLASS_WEIGHT[:c], 0)


def focal_held_to(case, dtype, kind, gout=1.0):
    """the same for the focal forms, against `restated`: fp32 evaluation of the restatement for the factor-4 term, its
    focal term on softmax (B) for the spread"""
    outs, onehot = inputs(case, dtype)
    spec = focal_spec(kind, onehot.shape[1])
    l64, g64 = restated_in(outs, onehot, spec, torch.float64)
    l32, g32 = restated_in(outs, onehot, spec, torch.float32)
    lb, gb = restated_in(outs, onehot, spec, torch.float64, softmax32=lambda z: softmax_b(z)[0].float())
    acc = [gout * (4.0 * float((a.double() - b).abs().max()) + float((c - b).abs().max())) for a, b, c in zip(g32, g64, gb)]
    return dict(loss64=l64, grads64=[g * gout for g in g64], acc=acc,
                loss_tol=4.0 * abs(l32 - l64) + abs(lb - l64) + 2.0 ** -24 * abs(l64))


def bias_conditions_met(ref64, dtype):
    """the conditions of hip_util.check_rounding_bias, evaluated on the reference: >= 10 000 elements at or above max/64,
    and >= 90 % of all"""
    _, used, n = signed_rounding_bias(ref64, ref64, dtype)
    return used >= 10000 and used >= 0.9 * n


def to_storage(ref64, dtype):
    """the fp64 reference rounded once, to nearest-even, into the storage type (what a faultless kernel stores)"""
    return ref64.to(TDT[dtype]).float() if dtype != F32 else ref64.float()
