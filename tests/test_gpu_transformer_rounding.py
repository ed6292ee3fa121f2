"""The transformer branches held to fp64 STAGE BY STAGE, as a plan runs them (teacher-forced), and the operator entries at
the edges tests/test_gpu_transformer_ops.py leaves out.

Teacher-forced: nothing here compares an end-to-end fp64 run with the device.  Every stage of tests/tf_ref.py is evaluated
in fp64 on the DEVICE'S OWN inputs to that stage, read back from the plan's workspace -- Runtime.read_region("tf_F",
"tf_save", "tf_tape", "tf_otape", "tf_dF"), Runtime.read_buffer("attnall", "g.attnall") -- and compared, element by
element, with the device's output of that stage.  Errors do not accumulate from stage to stage, so each stage gets the
bound of an operator test.  The plan runs forward in train mode and then the staged backward: stages = 3 (decoder, encoder,
UpConv chain) leaves g.attnall, the upstream gradient of the branches; stages = 4 runs the transformer backward on it.
plan.hip:hdf_plan_layout gives every one of these regions a range of its own in the arena (a bump allocator, nothing is
reused), tf_F / tf_save / attnall are read before the backward starts, and g.attnall is read between the two backward calls
AND after the second (asserted equal: the transformer backward only reads it).  What a training step runs is what is
checked: the default arrangement (the two persistent kernels of tf_chain_fwd.hip / tf_chain_bwd.hip where the shape allows), the
16-bit patch embedding and attention backward of the 16-bit plans, tf_wgrad over the tapes, the depth-1 patch embedding of
the 2-D model with its token-chunked float-atomic weight gradient (tf_patch_embed_bwd: kblocks = 2, tchunks = max(1,
min(ceil(B N / 256), 512 / (kblocks * ceil(DM / 32) * M))) = min(2, 32) = 2 at 256 x 256, batch 2, n_filters 16, 2
modalities) -- and one leg under HDF_NO_TF_CHAIN=1, so the fused launch chain is held on its own as well.

Bounds (hip_util.check_rounded / check_fp32_sum / check_rounding_bias).  The allowance of a stage is a property of the
reference alone: acc = FACTOR x max|stage in torch fp32 - stage in torch fp64| on the same inputs (tf_ref.acc_of; FACTOR
is 4 unless listed in tf_ref.FACTOR), per instance of the stage (modality, block, layer) and, for the attention tensors,
per head -- one head a thousand times smaller than the others is held as tightly as they are.  Where the kernel forms a
16-bit operand itself (P and dS in the attention backward of the 16-bit plans) the spread between the reference with that
operand formed in fp64 and in fp32 is added.  Sums taken with float atomics have no fixed order (bias / LayerNorm /
patch-bias gradients everywhere, the 2-D patch weight, every parameter gradient of the operator entries): their allowance
is the same FACTOR x spread of the column sum on the CPU plus 2^-24 x sum |terms|, per element, the terms taken in fp64 from
the device's own tape.  No element is excluded from any check.

Two allowances come from the number formats, not from a factor (tf_ref.attn_bwd_ambiguity; attention backward, tape
segment dq).  (1) D = dO v^T - (dO . ob) is the difference of two 4-term fp32 dot products and carries up to
4 * 2^-24 (sum |dO v| + sum |dO ob|) whatever is left of it: with one key D is exactly zero, the CPU's fp32 and fp64
evaluations agree to the last bit, and no fp32 kernel can.  (2) 16-bit plans: the kernel rounds its own fp32 P and dS to the
storage type.  An operand that lies within the fp32 evaluation error (4 x the CPU's fp32-vs-fp64 spread of P and of D) of a
rounding tie may round the other way than the reference's: one 16-bit ulp of that operand times the other operand, for
those operands only.  Measured without (2): dq elements of the bf16 plan were up to 1,819 x (f16: 281 x) outside a bound
of 4 x spread, each by one 16-bit ulp of one operand (2^-8 of a term against a spread of 1e-7), i.e. the rule "next power
of two above the worst ratio" would have set 2048 .. 8192 there -- a bound that a truncating rounding of EVERY
operand passes.  With (2) no element is outside at factor 4, and tests/test_tf_ref_cpu.py shows the truncation rejected.

MEASURED on an MI355X, worst error / bound over all cases, FACTOR 4 everywhere (in brackets: the factor at which the worst
element would sit exactly on its bound; the spread-independent parts of a bound -- half an ulp of the storage type, the
2^-24 terms, the two allowances above -- are taken off first, so 16-bit stores and atomics can show a ratio near 1 with a
small factor).  No stage needed a factor above 4: the hardware transcendentals of these kernels (v_exp_f32 on scores
pre-scaled by 0.5 log2 e, __logf, rsqrtf, __expf in the GELU derivative) stay within 3.2 x the CPU's spread -- the worst are
the attention output (2.91, f16 plan) and two weight gradients of the operator entries (3.14).  "plan": the five
plans and the launch-chain leg; "op.*": the operator entries.  Signed rounding bias of attnall: bf16 -0.0028 ulp, f16
+0.0021 ulp (bound 0.0096).

  op.attn: lse                           f32 0.41 (1.10)
  op.attn: ob                            f32 0.56 (2.24)
  op.attn: tape.dq                       f32 0.53 (2.09)   bf16 1.00 (0.10)   f16 0.94 (0.01)
  op.embed: embed                        f32 0.22 (0.86)
  op.embed: op.g.patch_embeddings.bias   f32 0.39 (0.55)
  op.embed: op.g.patch_embeddings.weight f32 0.24 (0.91)
  op.embed: op.g.position_embeddings     f32 0.22 (0.53)
  op.layer: feat                         f32 0.65 (2.57)
  op.layer: h0                           f32 0.66 (2.60)
  op.layer: h1                           f32 0.36 (1.31)
  op.layer: h2                           f32 0.36 (1.14)
  op.layer: lse                          f32 0.41 (1.33)
  op.layer: ob                           f32 0.67 (2.65)
  op.layer: op.dF                        f32 0.54 (2.15)
  op.layer: op.g.0.bias                  f32 0.29 (1.05)
  op.layer: op.g.0.weight                f32 0.53 (2.07)
  op.layer: op.g.1.fn.to_out.0.bias      f32 0.29 (0.78)
  op.layer: op.g.1.fn.to_out.0.weight    f32 0.32 (0.92)
  op.layer: op.g.1.fn.to_qkv.weight      f32 0.48 (1.93)
  op.layer: op.g.1.norm.bias             f32 0.44 (1.68)
  op.layer: op.g.1.norm.weight           f32 0.80 (3.14)
  op.layer: op.g.2.fn.net.0.bias         f32 0.34 (1.05)
  op.layer: op.g.2.fn.net.0.weight       f32 0.27 (0.70)
  op.layer: op.g.2.fn.net.3.bias         f32 0.21 (0.48)
  op.layer: op.g.2.fn.net.3.weight       f32 0.56 (1.99)
  op.layer: op.g.2.norm.bias             f32 0.27 (0.68)
  op.layer: op.g.2.norm.weight           f32 0.30 (0.86)
  op.layer: qkv                          f32 0.33 (1.16)
  op.out: attnall                        f32 0.62 (2.41)   bf16 1.00 (0.15)
  op.out: op.dF                          f32 0.69 (2.75)   bf16 0.42 (1.64)
  op.out: op.g.out_layer.net.0.bias      f32 0.43 (1.34)   bf16 0.50 (1.47)
  op.out: op.g.out_layer.net.0.weight    f32 0.66 (2.49)   bf16 0.47 (1.64)
  op.out: op.g.out_layer.net.3.bias      f32 0.28 (0.24)   bf16 0.18 (0.00)
  op.out: op.g.out_layer.net.3.weight    f32 0.82 (3.14)   bf16 0.64 (2.34)
  op.out: out                            f32 0.37 (1.36)
  plan: attnall                          f32 0.28 (1.08)   bf16 1.00 (0.22)   f16 0.99 (0.43)
  plan: dF0                              f32 0.34 (1.32)   bf16 0.27 (1.01)   f16 0.36 (1.34)
  plan: embed                            f32 0.12 (0.46)   bf16 0.06 (0.22)   f16 0.04 (0.15)
  plan: feat                             f32 0.40 (1.51)   bf16 0.38 (1.44)   f16 0.38 (1.43)
  plan: g.0.bias                         f32 0.29 (0.43)   bf16 0.22 (0.00)   f16 0.22 (0.00)
  plan: g.0.weight                       f32 0.25 (0.97)   bf16 0.21 (0.76)   f16 0.20 (0.63)
  plan: g.1.fn.to_out.0.bias             f32 0.39 (0.09)   bf16 0.26 (0.00)   f16 0.31 (0.00)
  plan: g.1.fn.to_out.0.weight           f32 0.31 (1.08)   bf16 0.25 (0.86)   f16 0.23 (0.74)
  plan: g.1.fn.to_qkv.weight             f32 0.29 (1.13)   bf16 0.25 (0.87)   f16 0.24 (0.94)
  plan: g.1.norm.bias                    f32 0.24 (0.39)   bf16 0.24 (0.12)   f16 0.28 (0.01)
  plan: g.1.norm.weight                  f32 0.28 (0.72)   bf16 0.38 (0.73)   f16 0.25 (0.22)
  plan: g.2.fn.net.0.bias                f32 0.66 (1.80)   bf16 0.27 (0.02)   f16 0.29 (0.28)
  plan: g.2.fn.net.0.weight              f32 0.44 (1.68)   bf16 0.57 (2.11)   f16 0.40 (1.52)
  plan: g.2.fn.net.3.bias                f32 0.47 (0.09)   bf16 0.39 (0.02)   f16 0.41 (0.37)
  plan: g.2.fn.net.3.weight              f32 0.50 (1.92)   bf16 0.33 (1.22)   f16 0.39 (1.53)
  plan: g.2.norm.bias                    f32 0.34 (0.44)   bf16 0.26 (0.14)   f16 0.24 (0.27)
  plan: g.2.norm.weight                  f32 0.41 (0.54)   bf16 0.34 (0.13)   f16 0.28 (0.19)
  plan: g.out_layer.net.0.bias           f32 0.22 (0.06)   bf16 0.26 (0.00)   f16 0.23 (0.00)
  plan: g.out_layer.net.0.weight         f32 0.29 (0.81)   bf16 0.17 (0.55)   f16 0.20 (0.55)
  plan: g.out_layer.net.3.bias           f32 0.21 (0.18)   bf16 0.18 (0.00)   f16 0.21 (0.00)
  plan: g.out_layer.net.3.weight         f32 0.28 (1.06)   bf16 0.14 (0.52)   f16 0.19 (0.66)
  plan: g.patch_embeddings.bias          f32 0.45 (1.05)   bf16 0.36 (0.35)   f16 0.49 (0.91)
  plan: g.patch_embeddings.weight        f32 0.40 (1.29)   bf16 0.24 (0.90)   f16 0.25 (0.93)
  plan: g.position_embeddings            f32 0.21 (0.19)   bf16 0.20 (0.00)   f16 0.20 (0.00)
  plan: h0                               f32 0.32 (1.18)   bf16 0.28 (1.06)   f16 0.28 (1.11)
  plan: h1                               f32 0.41 (1.42)   bf16 0.43 (1.61)   f16 0.41 (1.54)
  plan: h2                               f32 0.36 (1.39)   bf16 0.35 (1.36)   f16 0.38 (1.37)
  plan: lse                              f32 0.37 (1.12)   bf16 0.38 (1.19)   f16 0.40 (1.40)
  plan: ob                               f32 0.42 (1.67)   bf16 0.44 (1.77)   f16 0.73 (2.91)
  plan: otape.do                         f32 0.19 (0.72)   bf16 0.32 (1.17)   f16 0.21 (0.78)
  plan: otape.dz                         f32 0.50 (1.80)   bf16 0.33 (1.28)   f16 0.35 (1.41)
  plan: otape.f                          f32 0.48 (1.84)   bf16 0.43 (1.65)   f16 0.40 (1.56)
  plan: out                              f32 0.17 (0.64)   bf16 0.31 (1.22)   f16 0.36 (1.44)
  plan: qkv                              f32 0.37 (1.39)   bf16 0.33 (1.21)   f16 0.53 (2.03)
  plan: tape.dgo                         f32 0.36 (1.29)   bf16 0.36 (1.34)   f16 0.35 (1.35)
  plan: tape.dh0                         f32 0.33 (1.16)   bf16 0.32 (1.15)   f16 0.27 (0.93)
  plan: tape.dq                          f32 0.41 (1.25)   bf16 0.98 (0.20)   f16 0.86 (0.59)
  plan: tape.p0.dg                       f32 0.45 (1.69)   bf16 0.36 (1.20)   f16 0.40 (1.33)
  plan: tape.p0.dz                       f32 0.44 (1.67)   bf16 0.34 (1.12)   f16 0.34 (1.24)
  plan: tape.p0.f                        f32 0.48 (1.86)   bf16 0.30 (1.08)   f16 0.35 (1.29)
  plan: tape.p0.u                        f32 0.27 (0.88)   bf16 0.29 (0.96)   f16 0.32 (1.11)
  plan: tape.p1.dg                       f32 0.39 (1.34)   bf16 0.50 (1.77)   f16 0.42 (1.54)
  plan: tape.p1.dz                       f32 0.38 (1.41)   bf16 0.52 (2.02)   f16 0.70 (2.68)
  plan: tape.p1.f                        f32 0.27 (0.98)   bf16 0.33 (1.22)   f16 0.40 (1.47)
  plan: tape.p1.u                        f32 0.29 (1.01)   bf16 0.29 (0.94)   f16 0.28 (0.96)
  plan: tape.t                           f32 0.32 (1.11)   bf16 0.28 (0.88)   f16 0.25 (0.80)"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

import tf_ref
from hdf_rt._lib import BF16, F16, F32, check, lib, ptr
from hdf_rt.runtime import Plan, Runtime
from hip_util import DEV, TDT, check_fp32_sum, check_rounded, check_rounding_bias, rounding_excess, st, ulp_of
from oracle import detgen
from oracle import hdf_oracle as orc
from tf_ref import acc_of

pytestmark = pytest.mark.gpu
NAME = {F32: "f32", BF16: "bf16", F16: "f16"}
SEED = 1234
STRICT = True          # False (measuring scripts only): record the ratios without asserting


def _kind(name):
    """a parameter's name without its modality, block and layer: the stage a gradient check is reported under"""
    return re.sub(r"^attns\.\d+\.(blocks\.\d+\.0\.)?(layers\.\d+\.)?", "", name)


class Held:
    """the checks of one test: every call holds one tensor per element, report() prints one ROUNDING line per stage"""

    def __init__(self, case, dtype):
        self.case, self.dtype, self.worst, self.need, self.bad = case, dtype, {}, {}, {}

    def _note(self, stage, ratio, err, fixed, spread):
        self.worst[stage] = max(self.worst.get(stage, 0.0), float(ratio.max()))
        need = float(((err - fixed) / max(spread, 1e-300)).max()) if spread > 0 else 0.0
        self.need[stage] = max(self.need.get(stage, 0.0), need)
        n, k = self.bad.get(stage, (0, 0))
        self.bad[stage] = (n + int((ratio > 1).sum()), k + ratio.numel())

    def rounded(self, stage, got, ref64, ref32, dtype=F32, alt64=None, heads=0, what="", extra=None):
        """got: one rounding (to dtype) of a value within acc of ref64.  heads: width of a head's columns (0: one group);
        extra: a per-element allowance on top of the stage's (tf_ref.attn_bwd_ambiguity)"""
        got, ref64, ref32 = got.double().cpu(), ref64.double(), ref32.double()
        for s, acc in tf_ref.group_accs(stage, ref32, ref64, heads, alt64):
            g, r = got[..., s], ref64[..., s]
            rest = 0.0 if extra is None else extra[..., s]
            self._note(stage, rounding_excess(g, r, dtype, acc + rest), (g - r).abs(), 0.5 * ulp_of(r, dtype) + rest,
                       acc / tf_ref.FACTOR.get(stage, 4.0))
            if STRICT:
                check_rounded(g, r, dtype, acc + rest, "%s %s %s" % (self.case, stage, what))

    def summed(self, stage, got, ref64, ref32, terms=None, what=""):
        """got: an fp32 sum of exact products.  terms: sum |terms| per element where the sum has no fixed order"""
        got, ref64, ref32 = got.double().cpu(), ref64.double(), ref32.double()
        acc = acc_of(stage, ref32, ref64)
        extra = 0.0 if terms is None else 2.0 ** -24 * terms.double()
        bound = acc + extra + 2.0 ** -24 * ref64.abs()
        err = (got - ref64).abs()
        self._note(stage, err / bound.clamp_min(1e-300), err, extra + 2.0 ** -24 * ref64.abs(),
                   acc / tf_ref.FACTOR.get(stage, 4.0))
        if STRICT:
            check_fp32_sum(got, ref64, acc + extra, "%s %s %s" % (self.case, stage, what))

    def report(self):
        for stage in sorted(self.worst):
            print("ROUNDING %s.%s %s %.3f (factor to reach the bound: %.2f; outside: %d of %d)" % (
                self.case, stage, NAME[self.dtype], self.worst[stage], self.need[stage], self.bad[stage][0],
                self.bad[stage][1]))


# ================================================================================================ plan level
# (in_channels, n_cls, n_filters, image, depth, batch, dtype)
CASES = {
    "n8": (2, 3, 16, (32, 32, 32), 8, 2, F32),          # N = 8: one partial tile per sequence, two blocks
    "n27": (1, 2, 16, (48, 48, 48), 4, 3, F32),         # N = 27: a second, partial tile; odd batch
    "n64_bf16": (4, 4, 32, (64, 64, 64), 8, 2, BF16),   # N = 64: whole tiles; 16-bit patch embedding / attention backward
    "n64_f16": (4, 4, 32, (64, 64, 64), 8, 2, F16),
    "flat2d": (2, 2, 16, (256, 256), 4, 2, F32),        # the 2-D model: depth-1 patches, tchunks = 2 (float atomics)
}


def _params(plan, seed):
    """test_gpu_chain._params, with to_qkv.weight of block 0 four times larger (scores of tens) and the out-layer's output
    bias ten times larger"""
    g = torch.Generator().manual_seed(seed)
    flat = torch.zeros(plan.param_floats)
    for name, off, numel, shape in plan.table:
        if name.endswith("norm.weight") or (name.endswith(".weight") and len(shape) == 1):
            v = 1.0 + 0.1 * torch.randn(numel, generator=g)
        elif len(shape) > 1:
            fan = 1
            for s in shape[1:]:
                fan *= s
            v = torch.randn(numel, generator=g) / fan ** 0.5
        else:
            v = 0.1 * torch.randn(numel, generator=g)
        if ".blocks.0." in name and name.endswith("to_qkv.weight"):
            v = v * 4.0
        if name.endswith("out_layer.net.3.bias"):
            v = v * 10.0          # outputs off zero: the rounding-bias statistic of attnall needs 90 % of the elements
                                  # within a factor 64 of the largest
        flat[off:off + numel] = v
    return flat


@functools.lru_cache(maxsize=None)
def _run(key, chain=True):
    """forward (train mode), backward stages 3 then 4; everything the checks read, on the CPU"""
    cin, ncls, nf, image, depth, batch, dtype = CASES[key]
    if chain:
        os.environ.pop("HDF_NO_TF_CHAIN", None)
    else:
        os.environ["HDF_NO_TF_CHAIN"] = "1"
    try:
        plan = Plan(cin, ncls, nf, image, depth, dtype)
        rt = Runtime(plan, DEV)
        params = _params(plan, 1)
        x = torch.rand((batch, cin) + image, generator=torch.Generator().manual_seed(2))
        x = x + (0.6 * torch.arange(cin) - 0.3).view((1, cin) + (1,) * len(image))     # LayerNorm inputs off centre
        pd, xd = params.to(DEV), x.to(DEV)
        rt._ensure_ws(batch, True)
        rt.read_region("tf_sync").zero_()       # (the launch chain leaves the counters alone: no stale give-up word)
        pers, who = C.c_int(-1), C.c_int(-2)
        check(lib().hdf_plan_chain_state(plan.h, batch, C.byref(pers), C.byref(who)), "chain_state")
        outs = rt.forward(xd, pd, 1, SEED, need_backward=True)
        torch.cuda.synchronize()
        M, N, DM, nb = cin, 1, 4 * nf, depth // 4
        for s in image:
            N *= s // 16
        nseq = M * batch
        sync = rt.read_region("tf_sync").view(torch.int32)
        assert int(sync[32 * nseq]) == 0, "a per-sequence barrier of the persistent forward gave up (tf_sync word %d)" % int(
            sync[32 * nseq])
        res = {"plan": plan, "params": params, "x": x, "dims": (M, batch, N, DM, nb), "dtype": dtype,
               "persistent": pers.value,
               "F": tf_ref.read_F(rt.read_region("tf_F"), M, batch, N, DM, nb),
               "save": tf_ref.read_save(rt.read_region("tf_save"), M, batch, N, nb),
               "attnall": tf_ref.read_attnall(rt.read_buffer("attnall"), M, DM)}
        g = torch.Generator().manual_seed(5)
        douts = [(torch.randn(o.shape, generator=g) * 1e-2).to(DEV).to(o.dtype) for o in outs]
        grads = torch.zeros_like(pd)
        rt.backward(xd, pd, douts, grads, stages=3)
        torch.cuda.synchronize()
        gatt = rt.read_buffer("g.attnall")
        rt.backward(xd, pd, douts, grads, stages=4)
        torch.cuda.synchronize()
        sync = rt.read_region("tf_sync").view(torch.int32)
        assert int(sync[(1 << 17) + 32 * nseq]) == 0, "a per-sequence barrier of the persistent backward gave up"
        assert torch.equal(gatt, rt.read_buffer("g.attnall")), "the transformer backward changed g.attnall"
        res.update({"gatt": tf_ref.read_attnall(gatt, M, DM), "grads": grads.cpu(),
                    "tape": tf_ref.read_tape(rt.read_region("tf_tape"), M, batch, N, nb),
                    "otape": tf_ref.read_otape(rt.read_region("tf_otape"), M, batch, N, DM, nb),
                    "dF0": tf_ref.read_dF0(rt.read_region("tf_dF"), M, batch, N, DM)})
        return res
    finally:
        os.environ.pop("HDF_NO_TF_CHAIN", None)


def _sds(res):
    return (tf_ref.state_dict_of(res["plan"].table, res["params"], torch.float64),
            tf_ref.state_dict_of(res["plan"].table, res["params"], torch.float32))


def _layer_forward_held(h, sd64, sd32, drop, m, b, l, Fk, sv, feat):
    """the five stages of one dense layer, each from the DEVICE'S input to it.  Fk: F[:, 0:K]; sv: the saved tensors;
    feat: F[:, K:K+32] as the device wrote it"""
    lp, w = tf_ref.layer_prefix(m, b, l), "m%d b%d l%d" % (m, b, l)

    def site(kind):
        return detgen.site_id(m, b, l, kind)

    def both(fn, *a):
        return fn(*[t.double() for t in a], sd64), fn(*[t.float() for t in a], sd32)
    r64, r32 = both(lambda Fk_, sd: tf_ref.pre(Fk_, sd, lp)[0], Fk)
    h.rounded("h0", sv["h0"], r64, r32, what=w)
    r64, r32 = both(lambda h0, sd: tf_ref.qkv_of(h0, sd, lp)[1], sv["h0"])
    h.rounded("qkv", sv["qkv"], r64, r32, what=w)
    (o64, l64), (o32, l32) = tf_ref.attn_core(sv["qkv"].double()), tf_ref.attn_core(sv["qkv"].float())
    h.rounded("ob", sv["ob"], o64, o32, heads=4, what=w)
    h.rounded("lse", sv["lse"], l64, l32, what=w)
    r64, r32 = both(lambda ob, h0, sd: tf_ref.post_h1(ob, h0, sd, lp, drop, site(detgen.KIND_ATTN_OUT)), sv["ob"], sv["h0"])
    h.rounded("h1", sv["h1"], r64, r32, what=w)
    r64, r32 = both(lambda h1, sd: tf_ref.ff(h1, sd, lp, drop, site(detgen.KIND_FF1_A), site(detgen.KIND_FF1_B)) + h1,
                    sv["h1"])
    h.rounded("h2", sv["h2"], r64, r32, what=w)
    r64, r32 = both(lambda h2, sd: tf_ref.ff(h2, sd, lp, drop, site(detgen.KIND_FF2_A), site(detgen.KIND_FF2_B)), sv["h2"])
    h.rounded("feat", feat, r64, r32, what=w)


def _forward_held(key, res):
    M, B, N, DM, nb = res["dims"]
    dtype = res["dtype"]
    sd64, sd32 = _sds(res)
    drop = orc.Dropper(SEED)
    h = Held(key, dtype)
    kept = []
    for m in range(M):
        vol = res["x"][:, m:m + 1]
        h.rounded("embed", res["F"][0][m][..., :DM], tf_ref.patch_embed(vol.double(), sd64, m, drop, dtype),
                  tf_ref.patch_embed(vol, sd32, m, drop, dtype), what="m%d" % m)
        for b in range(nb):
            Fb = res["F"][b][m]
            for l in range(4):
                K = DM + 32 * l
                _layer_forward_held(h, sd64, sd32, drop, m, b, l, Fb[..., :K], res["save"][b][l][m], Fb[..., K:K + 32])
            bp = tf_ref.block_prefix(m, b)
            r64 = tf_ref.block_out(Fb.double(), sd64, bp, drop, m, b)
            r32 = tf_ref.block_out(Fb.float(), sd32, bp, drop, m, b)
            if b + 1 < nb:
                h.rounded("out", res["F"][b + 1][m][..., :DM], r64, r32, what="m%d b%d" % (m, b))
            else:
                h.rounded("attnall", res["attnall"][m], r64, r32, dtype=dtype, what="m%d" % m)
                live = r64 != 0                                    # (half of the elements are dropped: exact zeros)
                kept.append((res["attnall"][m][live], r64[live]))
    h.report()
    if dtype != F32:
        bias = check_rounding_bias(torch.cat([g for g, _ in kept]), torch.cat([r for _, r in kept]), dtype,
                                   "%s attnall" % key)
        print("ROUNDING %s.attnall.bias %s %+.4f ulp" % (key, NAME[dtype], bias))
    return h


def _dev_tapes(res, m):
    nb = res["dims"][4]
    return {"tape": [[res["tape"][b][l][m] for l in range(4)] for b in range(nb)],
            "otape": [res["otape"][b][m] for b in range(nb)]}


def _dev_forward(res, m):
    nb = res["dims"][4]
    return {"F": [res["F"][b][m] for b in range(nb)], "save": [[res["save"][b][l][m] for l in range(4)] for b in range(nb)]}


def _tape_held(h, stage, got, r64, r32, a64, what, amb=None):
    for k in ("dq", "t", "dh0", "dgo"):
        h.rounded(stage + k, got[k], r64[k], r32[k], alt64=None if (a64 is None or k != "dq") else a64[k],
                  heads=4 if k == "dq" else 0, what=what, extra=amb if k == "dq" else None)
    for p in ("p1", "p0"):
        for k in ("dg", "f", "dz", "u"):
            h.rounded("%s%s.%s" % (stage, p, k), got[p][k], r64[p][k], r32[p][k], what=what)


def _backward_held(key, res):
    M, B, N, DM, nb = res["dims"]
    dtype = res["dtype"]
    sd64, sd32 = _sds(res)
    drop = orc.Dropper(SEED)
    h = Held(key, dtype)
    for m in range(M):
        fw, dev = _dev_forward(res, m), _dev_tapes(res, m)
        args = [tf_ref.to_dtype(v, torch.float64) for v in (fw, res["gatt"][m], dev)]
        r64 = tf_ref.branch_backward(args[0], args[1], sd64, m, nb, drop, dtype, dev=args[2])
        a64 = (tf_ref.branch_backward(args[0], args[1], sd64, m, nb, drop, dtype, dev=args[2], form=torch.float32)
               if dtype != F32 else None)
        r32 = tf_ref.branch_backward(fw, res["gatt"][m], sd32, m, nb, drop, dtype, dev=dev)
        for b in range(nb):
            for k in ("do", "f", "dz"):
                h.rounded("otape." + k, dev["otape"][b][k], r64["otape"][b][k], r32["otape"][b][k], what="m%d b%d" % (m, b))
            for l in range(4):
                sv = args[0]["save"][b][l]     # the cancellation in dO v^T - delta; the 16-bit operands that sit on a tie
                dO = torch.matmul(args[2]["tape"][b][l]["dgo"], sd64[tf_ref.layer_prefix(m, b, l) + ".1.fn.to_out.0.weight"])
                amb = tf_ref.attn_bwd_ambiguity(sv["qkv"], sv["ob"], sv["lse"], dO, dtype, tf_ref.FACTOR.get("tape.dq", 4.0))
                _tape_held(h, "tape.", dev["tape"][b][l], r64["tape"][b][l], r32["tape"][b][l],
                           None if a64 is None else a64["tape"][b][l], "m%d b%d l%d" % (m, b, l), amb)
        h.rounded("dF0", res["dF0"][m], r64["dF0"], r32["dF0"], what="m%d" % m)
    h.report()
    return h


def _grads_held(key, res):
    """every parameter gradient of the branches against the fp64 contraction / column sum of the DEVICE'S tape operands"""
    M, B, N, DM, nb = res["dims"]
    sd64, sd32 = _sds(res)
    got = tf_ref.state_dict_of(res["plan"].table, res["grads"], torch.float32)
    drop = orc.Dropper(SEED)
    flat2d = res["x"].dim() == 4
    h = Held(key, res["dtype"])
    seen = set()
    for m in range(M):
        fw, dev = _dev_forward(res, m), _dev_tapes(res, m)
        vol = res["x"][:, m:m + 1]
        g64 = tf_ref.param_grads(tf_ref.to_dtype(fw, torch.float64), tf_ref.to_dtype(dev, torch.float64), sd64, m, nb)
        g32 = tf_ref.param_grads(fw, dev, sd32, m, nb)
        g64.update(tf_ref.embed_grads(vol.double(), res["dF0"][m].double(), sd64, m, drop))
        g32.update(tf_ref.embed_grads(vol, res["dF0"][m], sd32, m, drop))
        for name, (r64, terms) in g64.items():
            stage = "g." + _kind(name)
            matrix = r64.dim() >= 2 and "position" not in name
            # fixed-order sums: the weight matrices (tf_wgrad, <= 4096 tokens; the 3-D patch weight) and the position
            # gradient; float atomics: every vector, and the 2-D patch weight (token chunks)
            ordered = (matrix and not (flat2d and "patch" in name)) or "position" in name
            h.summed(stage, got[name].reshape(r64.shape), r64, g32[name][0], terms=None if ordered else terms, what=name)
            seen.add(name)
    assert seen == {n for n, _, _, _ in res["plan"].table if n.startswith("attns.")}
    h.report()
    return h


@pytest.mark.parametrize("key", list(CASES))
def test_plan_forward_stage_by_stage(key):
    _forward_held(key, _run(key))


@pytest.mark.parametrize("key", list(CASES))
def test_plan_backward_tapes_stage_by_stage(key):
    _backward_held(key, _run(key))


@pytest.mark.parametrize("key", list(CASES))
def test_plan_parameter_gradients_from_the_device_tapes(key):
    _grads_held(key, _run(key))


def test_the_default_arrangement_of_these_plans_is_the_persistent_one():
    """(what a training step runs; a plan that fell back to the launch chain would leave the persistent kernels unheld)"""
    for key in CASES:
        assert _run(key)["persistent"] == 1, key


def test_the_launch_chain_is_held_on_its_own():
    """HDF_NO_TF_CHAIN=1: the fused selections of tok_fwd_kernel / tok_bwd_kernel and the attention launches between them"""
    res = _run("n8", False)
    assert res["persistent"] == 0
    _forward_held("n8.nochain", res)
    _backward_held("n8.nochain", res)
    _grads_held("n8.nochain", res)


# ================================================================================================ operator level
NS = [1, 2, 15, 16, 17, 27]


def _ptr_array(tensors):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _pack(named, M):
    """[(state_dict suffix, [M, ...] tensor)] -> (flat [M * mstride], offsets, mstride): modality m at + m * mstride"""
    sizes = [int(np.prod(t.shape[1:])) for _, t in named]
    offs = np.concatenate([[0], np.cumsum([(s + 15) // 16 * 16 for s in sizes])]).astype(np.int64)
    mstride = int(offs[-1])
    flat = torch.zeros(M * mstride)
    for m in range(M):
        for (_, t), o, s in zip(named, offs, sizes):
            flat[m * mstride + o: m * mstride + o + s] = t[m].flatten()
    return flat, [int(o) for o in offs[:-1]], mstride


def _unpack(flat, named, offs, mstride, prefix, M):
    """flat buffer -> {prefix(m) + suffix: tensor}"""
    out = {}
    for m in range(M):
        for (sfx, t), o in zip(named, offs):
            n = int(np.prod(t.shape[1:]))
            out[prefix(m) + sfx] = flat[m * mstride + o: m * mstride + o + n].reshape(t.shape[1:])
    return out


def _gs(seed):
    return torch.Generator().manual_seed(seed)


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("nseq", [1, 3])
def test_attention_entries_peaked_scores_one_small_head(N, nseq):
    """hdf_op_attention_fwd / _bwd / _amp_bwd: max |score| about 60 on a common +40 per row; head 7's v and d_ob 1e-3 of the
    others'.  The backward is teacher-forced like the plan's: the reference takes the DEVICE'S ob and lse."""
    qkv, d_ob = tf_ref.attn_inputs(nseq, N, 100 * N + nseq, peaked=True)
    gq, gd = qkv.to(DEV).contiguous(), d_ob.to(DEV).contiguous()
    ob = torch.full((nseq, N, 32), float("nan"), device=DEV)
    lse = torch.full((nseq, N, 8), float("nan"), device=DEV)
    check(lib().hdf_op_attention_fwd(ptr(gq), nseq, N, ptr(ob), ptr(lse), st()), "attention_fwd")
    torch.cuda.synchronize()
    h = Held("op.attn.n%d.s%d" % (N, nseq), F32)
    (o64, l64), (o32, l32) = tf_ref.attn_core(qkv.double()), tf_ref.attn_core(qkv)
    h.rounded("ob", ob, o64, o32, heads=4)
    h.rounded("lse", lse, l64, l32)
    obc, lsec = ob.cpu(), lse.cpu()
    for dtype in (None, F32, BF16, F16):
        dq = torch.full((nseq, N, 96), float("nan"), device=DEV)
        if dtype is None:
            check(lib().hdf_op_attention_bwd(ptr(gq), ptr(ob), ptr(lse), ptr(gd), ptr(dq), nseq, N, st()), "attention_bwd")
        else:
            check(lib().hdf_op_attention_amp_bwd(dtype, ptr(gq), ptr(ob), ptr(lse), ptr(gd), ptr(dq), nseq, N, st()),
                  "attention_amp_bwd")
        torch.cuda.synchronize()
        dt = dtype or F32
        r64 = tf_ref.attn_bwd(qkv.double(), obc.double(), lsec.double(), d_ob.double(), dt)
        r32 = tf_ref.attn_bwd(qkv, obc, lsec, d_ob, dt)
        a64 = (tf_ref.attn_bwd(qkv.double(), obc.double(), lsec.double(), d_ob.double(), dt, form=torch.float32)
               if dt != F32 else None)
        hh = Held("op.attn.n%d.s%d%s" % (N, nseq, "" if dtype is not None else ".exact"), dt)
        amb = tf_ref.attn_bwd_ambiguity(qkv, obc, lsec, d_ob, dt, tf_ref.FACTOR.get("tape.dq", 4.0))
        hh.rounded("tape.dq", dq, r64, r32, alt64=a64, heads=4, extra=amb)
        hh.report()
    h.report()


LAYER_SFX = [".0.weight", ".0.bias", ".1.norm.weight", ".1.norm.bias", ".1.fn.to_qkv.weight", ".1.fn.to_out.0.weight",
             ".1.fn.to_out.0.bias", ".2.norm.weight", ".2.norm.bias", ".2.fn.net.0.weight", ".2.fn.net.0.bias",
             ".2.fn.net.3.weight", ".2.fn.net.3.bias"]


def _layer_params(DM, layer, M, seed):
    g = _gs(seed)
    K = DM + 32 * layer
    shapes = [(32, K), (32,), (32,), (32,), (96, 32), (32, 32), (32,), (32,), (32,), (64, 32), (64,), (32, 64), (32,)]
    out = []
    for i, s in enumerate(shapes):
        t = torch.randn((M,) + s, generator=g) * (s[1] ** -0.5 if len(s) == 2 else 0.1)
        if i in (2, 7):
            t = t + 1.0
        if i == 4:
            t = t * 4.0                      # scores of tens
        out.append(t)
    return list(zip(LAYER_SFX, out))


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("M,B", [(1, 1), (1, 3)])
def test_dense_layer_entry_tile_edges_and_gradient_buffers_that_start_non_zero(N, M, B):
    """hdf_op_dense_layer_fwd: every saved tensor from the device's input to its stage.  hdf_op_dense_layer_bwd: parameter
    gradients are ACCUMULATED (hdf.h) -- the buffers start at non-zero values -- and dF[:, 0:K] +=; held against the fp64
    backward of the layer on the device's saved tensors, plus what the buffers held"""
    DM, block, layer, seed = 64, 1, 2, 4242
    K, DMF, rows = DM + 32 * layer, DM + 128, B * N
    named = _layer_params(DM, layer, M, 7 * N + B)
    flat, offs, mstride = _pack(named, M)
    sd32 = _unpack(flat, named, offs, mstride, lambda m: tf_ref.layer_prefix(m, block, layer), M)
    sd64 = {k: v.double() for k, v in sd32.items()}
    Fin = torch.randn(M, B, N, DMF, generator=_gs(N)) + 0.5
    dFin = torch.randn(M, B, N, DMF, generator=_gs(N + 1))
    ginit = 0.1 * torch.randn(M * mstride, generator=_gs(N + 2))
    fd, gd = flat.to(DEV), ginit.to(DEV)
    pp, gp = [fd[o:] for o in offs], [gd[o:] for o in offs]
    Fd = Fin.to(DEV).contiguous()
    save = torch.zeros(M * rows * 232, device=DEV)
    check(lib().hdf_op_dense_layer_fwd(M, B, N, DM, block, layer, _ptr_array(pp), mstride, ptr(Fd), ptr(save), 1, seed,
                                       st()), "dense_layer_fwd")
    torch.cuda.synchronize()
    Fc = Fd.cpu()
    assert torch.equal(Fc[..., :K], Fin[..., :K]) and torch.equal(Fc[..., K + 32:], Fin[..., K + 32:])
    sv = tf_ref.read_save(save, M, B, N, 1, layers=1)[0][0]
    drop = orc.Dropper(seed)
    h = Held("op.layer.n%d.m%d.b%d" % (N, M, B), F32)
    for m in range(M):
        _layer_forward_held(h, sd64, sd32, drop, m, block, layer, Fc[m][..., :K], sv[m], Fc[m][..., K:K + 32])
    dFd = dFin.to(DEV).contiguous()
    scratch = torch.zeros(M * rows * 160, device=DEV)
    check(lib().hdf_op_dense_layer_bwd(M, B, N, DM, block, layer, _ptr_array(pp), _ptr_array(gp), mstride, ptr(Fd),
                                       ptr(dFd), ptr(save), ptr(scratch), 1, seed, st()), "dense_layer_bwd")
    torch.cuda.synchronize()
    dFc, gc = dFd.cpu(), gd.cpu()
    assert torch.equal(dFc[..., K:], dFin[..., K:])                 # read, not written
    got = _unpack(gc, named, offs, mstride, lambda m: tf_ref.layer_prefix(m, block, layer), M)
    init = _unpack(ginit, named, offs, mstride, lambda m: tf_ref.layer_prefix(m, block, layer), M)
    for m in range(M):
        lp = tf_ref.layer_prefix(m, block, layer)
        res = {}
        for wt, sd in ((torch.float64, sd64), (torch.float32, sd32)):
            svm = tf_ref.to_dtype(sv[m], wt)
            t = tf_ref.layer_backward(svm, dFin[m][..., K:K + 32].to(wt), sd, m, block, layer, drop)
            pg = tf_ref.layer_param_grads(Fc[m][..., :K].to(wt), svm, t, sd, lp)
            res[wt] = (t, pg, dFin[m][..., :K].to(wt) + torch.matmul(t["dh0"], sd[lp + ".0.weight"]))
        (t64, pg64, dF64), (t32, pg32, dF32) = res[torch.float64], res[torch.float32]
        h.rounded("op.dF", dFc[m][..., :K], dF64, dF32, what="m%d" % m)
        for name, (r64, terms) in pg64.items():
            i64, i32 = init[name].double(), init[name]
            h.summed("op.g." + _kind(name), got[name], i64 + r64, i32 + pg32[name][0], terms=terms + i64.abs(),
                     what=name)
    h.report()


OUT_SFX = [".out_layer.net.0.weight", ".out_layer.net.0.bias", ".out_layer.net.3.weight", ".out_layer.net.3.bias"]


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("M,B,last,dtype", [(1, 1, False, F32), (3, 1, True, F32), (1, 3, True, BF16)])
def test_block_out_entry_tile_edges_and_gradient_buffers_that_start_non_zero(N, M, B, last, dtype):
    """hdf_op_block_out_fwd / _bwd: next_F or the storage-typed attnall; the backward OVERWRITES dF (it starts as NaN here)
    and ACCUMULATES the parameter gradients (they start non-zero)"""
    DM, block, seed = 64, 1, 99
    DMF = DM + 128
    g = _gs(50 + N)
    named = list(zip(OUT_SFX, [torch.randn(M, 64, DMF, generator=g) * DMF ** -0.5, torch.randn(M, 64, generator=g) * 0.1,
                               torch.randn(M, DM, 64, generator=g) * 0.125, torch.randn(M, DM, generator=g) * 0.1]))
    flat, offs, mstride = _pack(named, M)
    sd32 = _unpack(flat, named, offs, mstride, lambda m: tf_ref.block_prefix(m, block), M)
    sd64 = {k: v.double() for k, v in sd32.items()}
    Fin = torch.randn(M, B, N, DMF, generator=g) + 0.5
    dout = torch.randn(M, B, N, DM, generator=g).to(TDT[dtype]).float()
    ginit = 0.1 * torch.randn(M * mstride, generator=g)
    fd, gd = flat.to(DEV), ginit.to(DEV)
    pp, gp = [fd[o:] for o in offs], [gd[o:] for o in offs]
    Fd = Fin.to(DEV).contiguous()
    drop = orc.Dropper(seed)
    h = Held("op.out.n%d.m%d.b%d" % (N, M, B), dtype)
    dF = torch.full((M, B, N, DMF), float("nan"), device=DEV)
    if last:
        attnall = torch.zeros(B, N, M * DM, dtype=TDT[dtype], device=DEV)
        check(lib().hdf_op_block_out_fwd(M, B, N, DM, block, _ptr_array(pp), mstride, ptr(Fd), None, ptr(attnall), dtype,
                                         1, seed, st()), "block_out_fwd")
        got = attnall.float().cpu().view(B, N, M, DM).permute(2, 0, 1, 3)
        d_att = dout.permute(1, 2, 0, 3).reshape(B, N, M * DM).to(TDT[dtype]).to(DEV).contiguous()
        check(lib().hdf_op_block_out_bwd(M, B, N, DM, block, _ptr_array(pp), _ptr_array(gp), mstride, ptr(Fd), None,
                                         ptr(d_att), dtype, ptr(dF), 1, seed, st()), "block_out_bwd")
    else:
        nxt = torch.zeros(M, B, N, DMF, device=DEV)
        check(lib().hdf_op_block_out_fwd(M, B, N, DM, block, _ptr_array(pp), mstride, ptr(Fd), ptr(nxt), None, dtype, 1,
                                         seed, st()), "block_out_fwd")
        got = nxt[..., :DM].cpu()
        dnext = torch.zeros(M, B, N, DMF)
        dnext[..., :DM] = dout
        dnext = dnext.to(DEV)
        check(lib().hdf_op_block_out_bwd(M, B, N, DM, block, _ptr_array(pp), _ptr_array(gp), mstride, ptr(Fd), ptr(dnext),
                                         None, dtype, ptr(dF), 1, seed, st()), "block_out_bwd")
    torch.cuda.synchronize()
    dFc = dF.cpu()
    gotg = _unpack(gd.cpu(), named, offs, mstride, lambda m: tf_ref.block_prefix(m, block), M)
    init = _unpack(ginit, named, offs, mstride, lambda m: tf_ref.block_prefix(m, block), M)
    for m in range(M):
        bp = tf_ref.block_prefix(m, block)
        h.rounded("attnall" if last else "out", got[m], tf_ref.block_out(Fin[m].double(), sd64, bp, drop, m, block),
                  tf_ref.block_out(Fin[m], sd32, bp, drop, m, block), dtype=dtype if last else F32, what="m%d" % m)
        o64 = tf_ref.out_backward(Fin[m].double(), dout[m].double(), sd64, m, block, drop)
        o32 = tf_ref.out_backward(Fin[m], dout[m], sd32, m, block, drop)
        h.rounded("op.dF", dFc[m], torch.matmul(o64["dz"], sd64[bp + OUT_SFX[0]]), torch.matmul(o32["dz"], sd32[bp + OUT_SFX[0]]),
                  what="m%d" % m)
        pg64, pg32 = tf_ref.out_param_grads(Fin[m].double(), o64, bp), tf_ref.out_param_grads(Fin[m], o32, bp)
        for name, (r64, terms) in pg64.items():
            i64, i32 = init[name].double(), init[name]
            h.summed("op.g." + _kind(name), gotg[name], i64 + r64, i32 + pg32[name][0], terms=terms + i64.abs(),
                     what=name)
    h.report()


@pytest.mark.parametrize("size", [(16, 16, 16), (16, 16, 32), (16, 48, 80), (32, 32, 64), (16, 16, 272), (48, 48, 48)],
                         ids=lambda s: "n%d" % (s[0] * s[1] * s[2] // 4096))
@pytest.mark.parametrize("M,B", [(1, 1), (2, 3)])
def test_patch_embed_bwd_accumulates_into_dweight_dpos_and_dbias(size, M, B):
    """hdf_op_patch_embed_fwd / _bwd at N = 1, 2, 15, 16, 17, 27.  The contract of include/hdf.h, pinned: ALL THREE gradients
    are added to what the buffers hold (patch_embed_wgrad_kernel: *q += acc; patch_embed_bwd_prep_kernel: dpos += s and an
    atomic add into dbias) -- hdf_backward zeroes the flat gradient buffer before any of them runs.  Every buffer starts at
    non-zero values; an entry that overwrote dweight would be off by exactly those."""
    D, H, W = size
    N, DM, seed = (D // 16) * (H // 16) * (W // 16), 64, 31337
    DMF = DM + 128
    g = _gs(DM + N)
    x = torch.rand(B, M, D, H, W, generator=g) + (0.6 * torch.arange(M) - 0.3).view(1, M, 1, 1, 1)
    named = [(".position_embeddings", torch.randn(M, 1, N, DM, generator=g) * 0.1),
             (".patch_embeddings.weight", torch.randn(M, DM, 1, 16, 16, 16, generator=g) * 4096 ** -0.5),
             (".patch_embeddings.bias", torch.randn(M, DM, generator=g) * 0.1)]
    flat, offs, mstride = _pack(named, M)
    sd32 = _unpack(flat, named, offs, mstride, lambda m: "attns.%d" % m, M)
    sd64 = {k: v.double() for k, v in sd32.items()}
    dF = torch.randn(M, B, N, DMF, generator=g)
    ginit = 0.1 * torch.randn(M * mstride, generator=g)
    fd, gd, xd = flat.to(DEV), ginit.to(DEV), x.to(DEV).contiguous()
    Fd = torch.zeros(M, B, N, DMF, device=DEV)
    check(lib().hdf_op_patch_embed_fwd(ptr(xd), M, B, D, H, W, DM, ptr(fd[offs[1]:]), ptr(fd[offs[2]:]), ptr(fd), mstride,
                                       ptr(Fd), 1, seed, st()), "patch_embed_fwd")
    dFd = dF.to(DEV)
    scratch = torch.zeros(M * B * N * DM, device=DEV)
    check(lib().hdf_op_patch_embed_bwd(ptr(xd), M, B, D, H, W, DM, ptr(dFd), mstride, ptr(gd[offs[1]:]), ptr(gd[offs[2]:]),
                                       ptr(gd), ptr(scratch), 1, seed, st()), "patch_embed_bwd")
    torch.cuda.synchronize()
    Fc = Fd.cpu()
    got = _unpack(gd.cpu(), named, offs, mstride, lambda m: "attns.%d" % m, M)
    init = _unpack(ginit, named, offs, mstride, lambda m: "attns.%d" % m, M)
    drop = orc.Dropper(seed)
    h = Held("op.embed.n%d.m%d.b%d" % (N, M, B), F32)
    for m in range(M):
        vol = x[:, m:m + 1]
        h.rounded("embed", Fc[m][..., :DM], tf_ref.patch_embed(vol.double(), sd64, m, drop),
                  tf_ref.patch_embed(vol, sd32, m, drop), what="m%d" % m)
        g64 = tf_ref.embed_grads(vol.double(), dF[m][..., :DM].double(), sd64, m, drop)
        g32 = tf_ref.embed_grads(vol, dF[m][..., :DM], sd32, m, drop)
        for name, (r64, terms) in g64.items():
            i64, i32 = init[name].double(), init[name]
            atomic = name.endswith("patch_embeddings.bias")          # (weight and position: one fixed-order sum, then +=)
            h.summed("op.g." + _kind(name), got[name], i64 + r64, i32 + g32[name][0],
                     terms=(terms + i64.abs()) if atomic else None, what=name)
    h.report()

