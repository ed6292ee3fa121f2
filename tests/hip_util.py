"""Helpers for the GPU parity tests: call the C ABI (through hdf_rt._lib) on torch tensors."""
import torch

from hdf_rt._lib import BF16, F16, F32, check, lib, ptr

TDT = {F32: torch.float32, BF16: torch.bfloat16, F16: torch.float16}
DEV = "cuda:0"


def st():
    return torch.cuda.current_stream().cuda_stream


def to_cl(x, dtype, cp=None):
    """[N,C,D,H,W] fp32 (cpu or gpu) -> channels-last storage tensor [N,D,H,W,CP] on the GPU."""
    n, c = x.shape[:2]
    cp = cp or c
    out = torch.zeros((n,) + tuple(x.shape[2:]) + (cp,), dtype=TDT[dtype], device=DEV)
    out[..., :c] = x.to(DEV).permute(0, 2, 3, 4, 1).to(TDT[dtype])
    return out.contiguous()


def from_cl(t):
    """channels-last [N,D,H,W,C] storage -> [N,C,D,H,W] fp32 on the CPU"""
    return t.float().permute(0, 4, 1, 2, 3).contiguous().cpu()


def rnd(x, dtype):
    """round a float tensor through the storage dtype"""
    return x.to(TDT[dtype]).float()


def pack_w(w, dtype, O, I, OP, IP, so, si, flip):
    dst = torch.empty(27 * OP * IP, dtype=TDT[dtype], device=DEV)
    wg = w.contiguous().to(DEV)
    check(lib().hdf_op_pack_weights(dtype, ptr(wg), ptr(dst), O, I, OP, IP, so, si, flip, st()), "pack")
    return dst


def rup(a, b):
    return (a + b - 1) // b * b


def conv3d(dtype, mode, x_cl, cin, w_packed, cout, bias=None, scale=None, shift=None, relu=0, stats=False,
           out=None, out_pitch=None, accumulate=0):
    n, d, h, w = x_cl.shape[:4]
    pitch = x_cl.shape[4]
    if mode == 0:
        od, oh, ow = d, h, w
    elif mode == 1:
        od, oh, ow = d // 2, h // 2, w // 2
    else:
        od, oh, ow = 2 * d, 2 * h, 2 * w
    if d == 1:
        od = 1          # depth 1 selects the 2-D operator: the depth axis is never strided
    if out is None:
        out = torch.zeros((n, od, oh, ow, cout), dtype=x_cl.dtype, device=DEV)
        out_pitch = cout
    part = None
    if stats:
        tiles = lib().hdf_op_conv3d_stat_tiles(dtype, cin, od, oh, ow)
        part = torch.zeros((n * tiles, rup(cout, 32), 2), dtype=torch.float32, device=DEV)
    check(lib().hdf_op_conv3d(dtype, mode, ptr(x_cl), pitch, cin, n, d, h, w, ptr(w_packed), ptr(bias), ptr(scale),
                              ptr(shift), relu, ptr(out), out_pitch, cout, ptr(part), accumulate, st()), "conv3d")
    return out, part


def rel_err(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / (b.norm() + 1e-30))


# ------------------------------------------------------------------------------------------------ rounding-aware checks
# A kernel that takes 16-bit operands, accumulates in fp32 and stores ONE rounding of the result may differ from the fp64
# value of the same expression by half a unit in the last place of the storage type plus the error of the fp32 accumulation
# -- nothing else.  These checks hold every element to that; rel_err (max error / max reference) does not see a truncating
# store, nor one voxel left out of a weight gradient.
SIG_BITS = {F32: 24, BF16: 8, F16: 11}        # significand bits, the implicit one included
MIN_EXP = {F32: -126, BF16: -126, F16: -14}   # exponent of the smallest normal; below it the spacing stays constant


def ulp_of(ref64, dtype):
    """spacing of the storage type at |ref64| (fp64 tensor): 2^(floor(log2|r|) - (bits - 1)), the subnormal spacing
    (2^-24 for float16) below the smallest normal and at zero"""
    _, e = torch.frexp(ref64.double().abs())                 # |r| = m * 2^e, m in [0.5, 1): floor(log2|r|) = e - 1
    e = torch.where(ref64 == 0, torch.full_like(e, MIN_EXP[dtype]), e - 1).clamp_min(MIN_EXP[dtype])
    return torch.exp2((e - (SIG_BITS[dtype] - 1)).double())


def rounding_excess(got, ref64, dtype, acc):
    """per element |got - ref64| / (0.5 ulp + acc): <= 1 where the element is one rounding of a value within acc of ref64"""
    got, ref64 = got.double(), ref64.double()
    assert got.shape == ref64.shape, (got.shape, ref64.shape)
    return (got - ref64).abs() / (0.5 * ulp_of(ref64, dtype) + acc)


def _worst(ratio, got, ref64, unit, unit_name, what):
    bad = ratio > 1.0
    flat = int(torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio).argmax())
    idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(flat), ratio.shape))
    g, r = float(got.double().flatten()[flat]), float(ref64.double().flatten()[flat])
    return ("%s: %d of %d elements outside the bound; worst at index %s: got %.9g, reference %.9g, error %.3f %s, "
            "%.3f x the bound" % (what, int(bad.sum()) + int(torch.isnan(ratio).sum()), ratio.numel(), idx, g, r,
                                  abs(g - r) / float(unit.flatten()[flat]), unit_name, float(ratio.flatten()[flat])))


def check_rounded(got, ref64, dtype, acc, what="output"):
    """assert, for EVERY element, |got - ref64| <= 0.5 * ulp_of(ref64, dtype) + acc.  got: the kernel's output (any float
    tensor, converted exactly to fp64); ref64: the fp64 reference on the storage-rounded operands; acc: an absolute
    allowance for the fp32 accumulation, taken from the reference alone (a number, or a tensor of per-element allowances).
    Returns the worst error / bound (<= 1)."""
    acc = torch.as_tensor(acc, dtype=torch.float64)
    assert bool((acc >= 0.0).all())          # (a NaN compares false)
    got, ref64 = got.double(), ref64.double()
    ratio = rounding_excess(got, ref64, dtype, acc)
    ok = bool((ratio <= 1.0).all())          # (a NaN compares false: a NaN output fails)
    assert ok, _worst(ratio, got, ref64, ulp_of(ref64, dtype), "ulp", what)
    return float(ratio.max())


def check_fp32_sum(got, ref64, acc, what="output"):
    """an fp32 result accumulated from exact products (the weight gradients): no storage rounding, so for EVERY element
    |got - ref64| <= acc + 2^-24 |ref64|.  acc: a number, or a tensor of per-element allowances (sums taken with float
    atomics: the order-dependent part 2^-24 * sum |terms| differs from element to element).  Returns the worst
    error / bound (<= 1)."""
    acc = torch.as_tensor(acc, dtype=torch.float64)
    assert bool((acc >= 0.0).all())          # (a NaN compares false)
    got, ref64 = got.double(), ref64.double()
    assert got.shape == ref64.shape, (got.shape, ref64.shape)
    bound = acc + 2.0 ** -24 * ref64.abs()
    ratio = (got - ref64).abs() / bound.clamp_min(1e-300)
    ok = bool((ratio <= 1.0).all())
    assert ok, _worst(ratio, got, ref64, bound.clamp_min(1e-300), "bounds", what)
    return float(ratio.max())


def signed_rounding_bias(got, ref64, dtype):
    """(bias, n_used, n): the mean of (got - ref64) * sign(ref64) / ulp over the elements with |ref64| >= max|ref64| / 64
    (below that the accumulation error is not small against the ulp).  Round-to-nearest-even gives 0 with standard
    deviation 0.289 / sqrt(n_used); a truncating store gives -0.5."""
    got, ref64 = got.double(), ref64.double()
    use = ref64.abs() >= ref64.abs().max() / 64
    e = ((got - ref64) * torch.sign(ref64) / ulp_of(ref64, dtype))[use]
    return float(e.mean()), int(use.sum()), ref64.numel()


def check_rounding_bias(got, ref64, dtype, what="output", expected=0.0):
    """a 16-bit output must be rounded without bias: |bias - expected| <= 6 sigma of round-to-nearest, on at least 90 % of
    the elements and at least 10 000 of them (conditions on the test's own data).  expected: the bias that rounding ref64
    itself to nearest-even has on this data (rne_bias), 0 where the fractions of an ulp that the rounding drops are
    uniformly distributed -- outputs of a long accumulation; not a softmax gradient of 16-bit logits, whose values cluster"""
    assert dtype in (BF16, F16)
    bias, used, n = signed_rounding_bias(got, ref64, dtype)
    assert used >= 0.9 * n and used >= 10000, "%s: the bias statistic uses %d of %d elements" % (what, used, n)
    assert abs(bias - expected) <= 6 * 0.289 / used ** 0.5, (
        "%s: signed rounding bias %.4f ulp over %d elements (round-to-nearest of the reference: %.4f, bound %.4f)" % (
            what, bias, used, expected, 6 * 0.289 / used ** 0.5))
    return bias


def rne_bias(ref64, dtype):
    """the signed rounding bias of ref64 rounded once, to nearest-even, into the storage type: a property of the data"""
    return signed_rounding_bias(ref64.double().to(TDT[dtype]), ref64, dtype)[0]
