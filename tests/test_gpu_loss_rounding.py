"""The fused loss kernels (csrc/loss.hip: loss_fwd / loss_bwd / focal_fwd / focal_bwd and their finalize) held to fp64 past
their grid cap: EVERY stored dlogits element of every scale within 0.5 ulp of the storage type (float16 subnormal spacing
included) + acc of the fp64 reference (hip_util.check_rounded; fp32 logits through the same call), the signed rounding bias
of the 16-bit gradients (hip_util.check_rounding_bias: a truncating store shows as -0.5 ulp), and the loss scalar.  The
golden tests of test_gpu_model.py allow 10 % of the maximum on 16-bit gradients at 16^3 voxels, where no thread takes a
second trip of its grid-stride loop; tests/test_loss_check_cpu.py shows what that lets through and that the checks here
reject it.

Reference: oracle/hdf_oracle.py deep_super_loss / ce_term / dice_term (tests/test_focal_loss_cpu.py `restated` for the focal
forms) with autograd in fp64 on the storage-rounded logits.  The allowances are properties of the reference alone
(tests/loss_ref.py held_to), never of the kernels' output:
  acc_i    = 4 max|grad_i(reference in fp32) - grad_i(reference in fp64)|
             + max|grad_i(A) - grad_i(B)|, the fp64 closed-form gradient kce (p - onehot) + p (G - <G, p>) with the softmax
             formed (A) in fp64 and (B) as the kernels' fast intrinsics form it, emulated in fp32 on the CPU:
             exp2(fl(x * log2 e)), ln2 * log2(s), 1 / se then a multiply
  loss_tol = 4 |loss(reference in fp32) - loss64| + |loss(A) - loss(B)| + 2^-24 |loss64|
The rounding bias is taken where the REFERENCE gradient meets the statistic's conditions (>= 10 000 elements, >= 90 % of
them >= max/64): the cases past the cap with N(0,1) logits, not logits x 30.  It is measured against the bias that rounding
the fp64 reference itself to nearest-even has on the same data (hip_util.rne_bias, a property of the reference): the
softmax of 16-bit logits takes clustered values, and over 10^5 .. 10^7 elements the correctly rounded reference shows up
to 0.011 ulp of signed bias of its own (cap_2d bf16; -0.0007 ulp at cap_vec4 bf16, where 6 sigma is 0.0006; -0.017 ulp on
float16 subnormals of a handful of ulp each) -- tests/test_loss_check_cpu.py.  A truncating store is -0.5 ulp either way.
The unscaled float16 cap_vec4 gradient is subnormal throughout: a store that flushes subnormals fails both checks there;
the x 65 536 case (GradScaler's initial scale) is the same gradient in normal numbers.

Out of scope: NaN / Inf logits (torch's softmax and the kernels' max-subtracted fast exp differ there by design).

route -> case (each for f32, bf16, f16 unless said otherwise):
  vec-4 body, second trip (V0 = 1 105 920 > 1024 x 256 x 4); widths 120/60/30/15 -> vec 4,4,1,1 in one launch; 4 class slots
                                             test_ce_dice[cap_vec4-*]  (12 forms: (w_ce, w_dice) x class weight x ignore)
  vec-1 body, second trip (widths 66/33, V0 = 270 336 > 1024 x 256); 8 class slots     test_ce_dice[cap_vec1-*]
  depth-1 (2-D) form, vec 1, 264 196 voxels                                              test_ce_dice[cap_2d-*]
  vec 1 chosen by alignment (logits and target one element off 16 bytes), past the cap   test_ce_dice[cap_unaligned-*]
  widths 24/12/6/3, batch 3                                                              test_ce_dice[small_odd-*] (12 forms)
  2 and 8 classes                                                                        test_ce_dice[c2-*], [c8-*]
  a class absent from the target, one never the argmax (U -> smooth only)               test_ce_dice[absent-*]
  logits x 30: exp underflows, gradient exactly 0 or +-k                                 test_ce_dice[saturated-*]
  grad_out 0.37; 65 536 on float16                                                       test_grad_out[...]
  focal_fwd / focal_bwd, FocalLoss(0.25, 2, 'sum') and FLPlusDice, bf16 and f16          test_focal[focal_vec4-*], [cap_vec1-*]
  hdf_loss_forward/_backward == hdf_loss_terms_*(1, 1) == hdf_loss_weighted_*(1, 1, NULL, 0), bit for bit
                                                                                         test_c_entries_agree_bit_for_bit
  two calls of one entry at cap_vec4, bit for bit                                        test_two_calls_are_bit_identical
Each check prints "ROUNDING <case> <dtype> <worst error / bound>" (pytest -s).  Worst ratio per case on an MI355X:
(worst over the forms of a case; a 16-bit dlogits ratio reaches 1.000 by construction -- the bound is half an ulp and
roundings come arbitrarily close to a tie -- so the fp32 column is the one that shows the slack of the arithmetic;
cap_2d bf16 is not in this recording)
  cap_vec4.dlogits             f32 0.287  bf16 1.000  f16 1.000
  cap_vec4.loss                f32 0.428  bf16 0.197  f16 0.183
  cap_vec1.dlogits             f32 0.224  bf16 0.999  f16 1.000
  cap_vec1.loss                f32 0.181  bf16 0.080  f16 0.160
  cap_2d.dlogits               f32 0.207  f16 1.000
  cap_2d.loss                  f32 0.138  f16 0.201
  cap_unaligned.dlogits        f32 0.224  bf16 0.999  f16 1.000
  cap_unaligned.loss           f32 0.160  bf16 0.017  f16 0.153
  small_odd.dlogits            f32 0.466  bf16 1.000  f16 0.998
  small_odd.loss               f32 0.187  bf16 0.169  f16 0.188
  c2.dlogits                   f32 0.273  bf16 0.998  f16 0.996
  c2.loss                      f32 0.175  bf16 0.403  f16 0.234
  c8.dlogits                   f32 0.238  bf16 0.999  f16 0.998
  c8.loss                      f32 0.182  bf16 0.087  f16 0.107
  absent.dlogits               f32 0.214  bf16 1.000  f16 0.997
  absent.loss                  f32 0.148  bf16 0.079  f16 0.163
  saturated.dlogits            f32 0.211  bf16 0.999  f16 0.997
  saturated.loss               f32 0.068  bf16 0.195  f16 0.208
  small_oddx0.37.dlogits       bf16 1.000
  small_oddx0.37.loss          bf16 0.016
  cap_vec4x65536.dlogits       f16 0.996
  cap_vec4x65536.loss          f16 0.183
  cap_vec1x65536.dlogits       f16 0.995
  cap_vec1x65536.loss          f16 0.053
  focal_vec4[focal].dlogits    bf16 0.996  f16 0.944
  focal_vec4[focal].loss       bf16 0.000  f16 0.148
  cap_vec1[focal].dlogits      bf16 0.998  f16 0.989
  cap_vec1[focal].loss         bf16 0.370  f16 0.280
  focal_vec4[flpd].dlogits     bf16 1.000  f16 1.000
  focal_vec4[flpd].loss        bf16 0.340  f16 0.149
  cap_vec1[flpd].dlogits       bf16 0.999  f16 1.000
  cap_vec1[flpd].loss          bf16 0.463  f16 0.118
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import loss_ref as lr  # noqa: E402
from hdf_rt._lib import BF16, F16, F32, check, lib, ptr  # noqa: E402
from hip_util import DEV, TDT, check_rounded, check_rounding_bias, rne_bias, st  # noqa: E402

ALL = [F32, BF16, F16]
TWELVE = ("cap_vec4", "small_odd")
CE_DICE = [(case, dtype, form) for case in ("cap_vec4", "cap_vec1", "cap_2d", "cap_unaligned", "small_odd", "c2", "c8",
                                             "absent", "saturated")
           for dtype in ALL for form in (lr.FORMS if case in TWELVE else (lr.DEFAULT, lr.WEIGHTED))]


def _id(v):
    return v if isinstance(v, str) else lr.form_name(v) if isinstance(v, tuple) else lr.NAME.get(v, str(v))


def _off_by_one(x):
    """a contiguous view of the same values that starts one element into its storage (2 or 4 bytes off 16)"""
    buf = torch.zeros(x.numel() + 8, dtype=x.dtype, device=x.device)
    v = buf[1:1 + x.numel()].view(x.shape)
    v.copy_(x)
    assert v.is_contiguous() and v.data_ptr() % 16 != 0
    return v


def _device_inputs(case, dtype):
    outs, onehot = lr.inputs(case, dtype)
    d = [o.to(DEV).to(TDT[dtype]) for o in outs]
    t = onehot.to(DEV)
    if lr.CASES[case][4].get("unaligned"):
        d, t = [_off_by_one(o) for o in d], _off_by_one(t)
    return [o.requires_grad_(True) for o in d], t


def _held(case, dtype, h, loss, grads):
    """every element of every dlogits, the bias where the reference allows the statistic, the loss scalar"""
    worst = 0.0
    for i, (g, r, acc) in enumerate(zip(grads, h["grads64"], h["acc"])):
        what = "%s dlogits%d" % (case, i)
        assert g.dtype == TDT[dtype]
        got = g.detach().float().cpu()
        worst = max(worst, check_rounded(got, r, dtype, acc, what))
        if dtype != F32 and lr.bias_conditions_met(r, dtype):
            check_rounding_bias(got, r, dtype, what, expected=rne_bias(r, dtype))
    print("ROUNDING %s.dlogits %s %.3f" % (case, lr.NAME[dtype], worst))
    ratio = abs(loss - h["loss64"]) / h["loss_tol"]
    print("ROUNDING %s.loss %s %.3f" % (case, lr.NAME[dtype], ratio), flush=True)
    assert ratio <= 1.0, "%s: loss %.9g, reference %.9g, allowed %.3e" % (case, loss, h["loss64"], h["loss_tol"])


def _run_ce_dice(case, dtype, form, gout):
    from hdf_rt.loss_fn import DeepSuperCEDice
    outs, tgt = _device_inputs(case, dtype)
    cw = lr.form_weight(form, tgt.shape[1], torch.float32)
    loss = DeepSuperCEDice.apply((tgt, form[0], form[1], cw, form[3]), *outs)
    loss.backward(torch.tensor(gout, device=DEV))
    _held("%s[%s]" % (case, lr.form_name(form)) + ("" if gout == 1.0 else "x%g" % gout), dtype,
          lr.held_to(case, dtype, form, gout), float(loss.detach()), [o.grad for o in outs])


@pytest.mark.parametrize("case,dtype,form", CE_DICE, ids=_id)
def test_ce_dice(case, dtype, form):
    _run_ce_dice(case, dtype, form, 1.0)


@pytest.mark.parametrize("case,dtype,gout", [("small_odd", BF16, 0.37), ("cap_vec4", F16, 65536.0),
                                             ("cap_vec1", F16, 65536.0)], ids=_id)
def test_grad_out(case, dtype, gout):
    """65 536 is GradScaler's initial scale: the float16 gradient past the cap in normal numbers (unscaled, 1 / (2 x
    1 105 920) voxels is subnormal)"""
    _run_ce_dice(case, dtype, lr.DEFAULT, gout)


@pytest.mark.parametrize("case", ["focal_vec4", "cap_vec1"])
@pytest.mark.parametrize("dtype", [BF16, F16], ids=_id)
@pytest.mark.parametrize("kind", ["focal", "flpd"])
def test_focal(kind, dtype, case):
    from hdf_rt.loss_fn import DeepSuperFocalDice
    outs, tgt = _device_inputs(case, dtype)
    w_focal, alpha, gamma, red, w_dice, weight, ignore = lr.focal_spec(kind, tgt.shape[1])
    cw = None if weight is None else torch.tensor(weight)
    loss = DeepSuperFocalDice.apply((tgt, w_focal, alpha, gamma, red, w_dice, cw, ignore), *outs)
    loss.backward()
    _held("%s[%s]" % (case, kind), dtype, lr.focal_held_to(case, dtype, kind), float(loss.detach()),
          [o.grad for o in outs])


# ------------------------------------------------------------------------------------------------ the C entries themselves
ENTRIES = {"hdf_loss_": (), "hdf_loss_terms_": (1.0, 1.0), "hdf_loss_weighted_": (1.0, 1.0, None, 0)}


def _c_loss(entry, dtype, outs, tgt):
    """one forward + backward through the C ABI -> (loss tensor, [dlogits]); the outputs start out as NaN"""
    n = len(outs)
    b, c = tgt.shape[:2]
    sp = tuple(tgt.shape[2:])
    d, h, w = ((1,) + sp) if len(sp) == 2 else sp
    ws = torch.zeros(lib().hdf_loss_workspace_bytes(b), dtype=torch.uint8, device=DEV)
    loss = torch.full((), float("nan"), dtype=torch.float32, device=DEV)
    douts = [torch.full_like(o, float("nan")) for o in outs]
    gout = torch.ones(1, dtype=torch.float32, device=DEV)
    po = [ptr(o) for o in outs] + [None] * (4 - n)
    pd = [ptr(o) for o in douts] + [None] * (4 - n)
    head = (dtype, po[0], po[1], po[2], po[3], n, ptr(tgt), b, c, d, h, w) + ENTRIES[entry]
    check(getattr(lib(), entry + "forward")(*head, ptr(ws), ptr(loss), st()), entry + "forward")
    check(getattr(lib(), entry + "backward")(*head, ptr(ws), ptr(gout), pd[0], pd[1], pd[2], pd[3], st()),
          entry + "backward")
    torch.cuda.synchronize()
    return loss, douts


@pytest.mark.parametrize("dtype", ALL, ids=_id)
def test_c_entries_agree_bit_for_bit(dtype):
    """include/hdf.h: hdf_loss_weighted_* with (NULL, 0) "reproduce hdf_loss_terms_* bit for bit", and (1, 1) is
    hdf_loss_forward / _backward; the autograd node calls the weighted entries"""
    from hdf_rt.loss_fn import DeepSuperCEDice
    outs, tgt = _device_inputs("small_odd", dtype)
    with torch.no_grad():
        res = {e: _c_loss(e, dtype, [o.detach() for o in outs], tgt) for e in ENTRIES}
    loss = DeepSuperCEDice.apply(tgt, *outs)
    loss.backward()
    l0, g0 = res["hdf_loss_"]
    assert len(g0) == 4 and not bool(torch.isnan(l0))
    for e, (l, g) in res.items():
        assert torch.equal(l, l0), e
        assert all(torch.equal(a, b) for a, b in zip(g, g0)), e      # (NaN never equals: every element was written)
    assert torch.equal(loss.detach(), l0) and all(torch.equal(o.grad, b) for o, b in zip(outs, g0))


@pytest.mark.parametrize("dtype", ALL, ids=_id)
def test_two_calls_are_bit_identical(dtype):
    """the sums of a thread are taken in voxel order, of a block and of the finalize in a fixed order: past the cap too"""
    outs, tgt = _device_inputs("cap_vec4", dtype)
    outs = [o.detach() for o in outs]
    la, ga = _c_loss("hdf_loss_weighted_", dtype, outs, tgt)
    lb, gb = _c_loss("hdf_loss_weighted_", dtype, outs, tgt)
    assert torch.equal(la, lb) and all(torch.equal(a, b) for a, b in zip(ga, gb))
