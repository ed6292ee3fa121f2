"""The 16-bit (and, where the entry takes it, fp32) operator kernels held to their ROUNDING: every element of a kernel's
output against an fp64 reference of the same operation on the storage-rounded operands (hip_util.check_rounded:
|got - ref64| <= 0.5 ulp of the storage type + acc), the signed rounding bias of 16-bit outputs
(hip_util.check_rounding_bias: a truncating store shows as -0.5 ulp), and fp32 weight gradients with no rounding term at
all (hip_util.check_fp32_sum: |got - ref64| <= acc + 2^-24 |ref64|).  The operator tests of test_gpu_ops.py,
test_gpu_ops_2d.py and test_gpu_ops_random_shapes.py use max error / max reference at 2e-2 (bf16) and 3e-3 (float16),
which neither a truncating store nor a voxel left out of a weight gradient exceeds (tests/test_rounding_check_cpu.py).

acc, the allowance for fp32 accumulation, comes from the reference alone, never from the kernel's output:
acc = 4 * max|op in torch fp32 - op in torch fp64| on the same rounded operands (both the CPU's fp32 op and the MFMA loop
sum products that are exact in fp32; they differ in order and K split, which is what the 4 is for).  Where a kernel forms
an operand itself and rounds it to 16 bits (the producer's relu(x * scale + shift) on load, the InstanceNorm backward inside
a weight gradient), an fp32 fma against mul + add, or a sum taken in another order, can turn a rounding the other way: the
reference is evaluated with the operand formed in fp64 and in unfused fp32, and max|op(A) - op(B)| is added to acc.
No case needed a factor above 4.  One reference is not torch's own fp32 op: the head's dweight / dbias are sums of 8- and
11-bit terms that torch's blocked fp32 reduction takes exactly, so the fp32 side there is the plain term-after-term sum.

Statistics partials (csrc/conv_igemm.hip, conv_wr.hip, conv_first.hip epilogues): every kernel sums the fp32 value
conv + bias BEFORE the rounding to the storage type (include/hdf.h at hdf_op_conv3d); the rows, summed in fp64, are held
per (n, c) to 4 * the fp32-vs-fp64 spread of the same per-channel sums of the reference on the CPU.  hdf_op_conv3d_bwd_stats
sums the STORED gradient (hdf.h), so its rows are checked against sums of the output itself.

route -> case (every case for bf16 and float16; "+f32" where fp32 storage runs too):
  conv_igemm, stride 1                      test_conv_forward[igemm_s1]                       +f32
  conv_ws2_kernel, ragged / whole tiles     test_conv_forward[ws2_ragged], [ws2_whole]        +f32
  input transform + channel-slice pitches   test_conv_forward[xf_pitch_small], [xf_pitch_ws2] +f32
  hdf_op_conv3d_split                       test_conv_split_output (conv_igemm and conv_ws2)  +f32
  hdf_op_conv3d_wr (K split over waves)     test_conv_forward[wr], [wr_accumulate_pitch]
  hdf_op_conv3d_first                       test_conv_first_layer (Cin 4 and 1, bias on / off)
  stride 2, generic / whole tiles           test_conv_forward[s2_generic] (+f32), [s2_whole]
  transposed, generic / whole / odd         test_conv_forward[t_generic] (+f32), [t_whole], [t_whole_xf], [t_odd], [s2_odd]
  accumulate = 1                            test_conv_forward[acc_igemm], [acc_ws2] (+f32), [wr_accumulate_pitch]
  2-D forms of the three modes              test_conv_forward[flat_s1], [flat_s2], [flat_t]   +f32
  hdf_op_conv3d_wgrad                       test_weight_gradient[...]                         +f32
  hdf_op_conv3d_first_wgrad / _wgrad_in     test_first_layer_weight_gradient, test_first_layer_weight_gradient_norm_inside
  hdf_op_in_bwd_wgrad                       test_norm_backward_inside_weight_gradient
  hdf_op_conv3d_bwd_stats                   test_data_gradient_with_norm_backward_rows
  hdf_op_in_bwd                             test_instance_norm_backward                       +f32
  hdf_op_norm_relu_add, enc_tail(_up)       test_norm_relu_add, test_encoder_tail, test_encoder_tail_up   +f32
  hdf_op_upsample_fwd / _bwd                test_upsample                                     +f32
  hdf_op_maxpool_bwd, accumulate = 1        test_maxpool_backward_accumulate                  +f32
  2-D pool family (hdf_op_enc_tail_2d, _maxpool_bwd_in_2d, _upsample_fwd_2d / _bwd_2d) and hdf_op_in_finalize
                                            tests/test_gpu_pool2d_rounding.py                 +f32
  hdf_op_head_fwd / _bwd                    test_head                                         +f32
  hdf_op_block_out_fwd, attnall             test_block_out_attnall
  hdf_optim_step, hdf_adam_step, Flat*      tests/test_gpu_optim_rounding.py (fp32 only; bound: tests/optim_ref.py)
Each check prints one line "ROUNDING <case> <worst error / bound>" (pytest -s shows them)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from hdf_rt._lib import BF16, F16, F32, check, lib, ptr  # noqa: E402
from hip_util import (DEV, TDT, check_fp32_sum, check_rounded, check_rounding_bias, from_cl, pack_w, rnd, rup, st,  # noqa: E402
                      to_cl)

NAME = {F32: "f32", BF16: "bf16", F16: "f16"}
ALL, HALF = [F32, BF16, F16], [BF16, F16]


def _mk(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _bc(v):
    return v[:, :, None, None, None]


def _acc(ref32, ref64, factor=4.0):
    """the accumulation allowance: a property of the reference alone"""
    return factor * float((ref32.double() - ref64).abs().max())


def _held(case, dtype, got, ref64, acc, bias=True):
    """16-bit (or fp32) output against the fp64 reference: every element, then the signed bias of the 16-bit roundings"""
    worst = check_rounded(got, ref64, dtype, acc, case)
    if bias and dtype != F32:
        check_rounding_bias(got, ref64, dtype, case)
    print("ROUNDING %s %s %.3f" % (case, NAME[dtype], worst))


def _held_sum(case, dtype, got, ref64, acc):
    print("ROUNDING %s %s %.3f" % (case, NAME[dtype], check_fp32_sum(got, ref64, acc, case)))


def _operand(x, scale, shift, dtype):
    """relu(x * scale + shift) rounded to the storage type, formed (A) in fp64 -- what an fp32 fma gives -- and (B) by an
    fp32 multiply and add"""
    a = torch.relu(x.double() * _bc(scale).double() + _bc(shift).double()).float()
    b = torch.relu(x * _bc(scale) + _bc(shift))
    return rnd(a, dtype), rnd(b, dtype)


def _stats_held(case, dtype, rows64, ref32, ref64, dims):
    """partial rows summed in fp64, [n, c, 2], against the per-channel sum and sum of squares of the fp32 results"""
    for j, (r32, r64) in enumerate(((ref32, ref64), (ref32 * ref32, ref64 * ref64))):
        want = r64.sum(dims)
        tol = 4 * float((r32.sum(dims).double() - want).abs().max())
        err = (rows64[..., j] - want).abs()
        assert bool((err <= tol).all()), "%s: statistic %d of (n, c) %s off by %.3e, allowed %.3e" % (
            case, j, tuple(int(v) for v in torch.unravel_index(err.argmax(), err.shape)), float(err.max()), tol)
        print("ROUNDING %s.stat%d %s %.3f" % (case, j, NAME[dtype], float(err.max()) / max(tol, 1e-300)))


# ------------------------------------------------------------------------------------------------ forward convolutions
def _torch_conv(mode, flat):
    if flat:
        return [lambda x, w, b: F.conv2d(x, w, b, padding=1), lambda x, w, b: F.conv2d(x, w, b, stride=2, padding=1),
                lambda x, w, b: F.conv_transpose2d(x, w, b, stride=2, padding=1, output_padding=1)][mode]
    return [lambda x, w, b: F.conv3d(x, w, b, padding=1), lambda x, w, b: F.conv3d(x, w, b, stride=2, padding=1),
            lambda x, w, b: F.conv_transpose3d(x, w, b, stride=2, padding=1, output_padding=1)][mode]


def _embed(w):
    """2-D weight [A, B, 3, 3] -> the 27-tap panel's layout with the kernel on the centre depth plane"""
    w3 = torch.zeros(w.shape[0], w.shape[1], 3, 3, 3)
    w3[:, :, 1] = w
    return w3


def _pack(w, dtype, mode, cin, cout, flat):
    w3 = _embed(w) if flat else w
    if mode == 2:
        return pack_w(w3, dtype, cout, cin, rup(cout, 32), cin, 27, cout * 27, 0)
    return pack_w(w3, dtype, cout, cin, rup(cout, 32), cin, cin * 27, 27, 0)


# name: (dtypes, mode, cin, cout, size, n, options)
#   bias / xf (input transform) / acc (out += conv) / stats / in2 (input = upper half of a 2*Cin row) /
#   out (pitch in units of Cout, leading channels in units of Cout) / wr (hdf_op_conv3d_wr) / flat (depth 1)
FWD = {
    "igemm_s1": (ALL, 0, 32, 32, (12, 16, 24), 2, dict(bias=1, stats=1)),
    "ws2_ragged": (ALL, 0, 16, 48, (49, 51, 53), 2, dict(bias=1, stats=1)),
    "ws2_whole": (ALL, 0, 32, 32, (48, 56, 64), 2, dict(bias=1, stats=1)),
    "xf_pitch_small": (ALL, 0, 32, 32, (8, 16, 8), 2, dict(xf=1, in2=1, out=(3, 1))),
    "xf_pitch_ws2": (ALL, 0, 32, 32, (48, 48, 56), 2, dict(xf=1, in2=1, out=(3, 1))),
    "wr": (HALF, 0, 64, 32, (64, 56, 48), 2, dict(bias=1, stats=1, wr=1)),
    "wr_accumulate_pitch": (HALF, 0, 64, 32, (48, 48, 56), 2, dict(acc=1, in2=1, out=(3, 1), wr=1)),
    "s2_generic": (ALL, 1, 32, 64, (16, 8, 12), 2, dict()),
    "s2_whole": (HALF, 1, 32, 64, (16, 16, 24), 2, dict(bias=1)),
    "s2_odd": (HALF, 1, 32, 63, (8, 8, 16), 2, dict()),
    "t_generic": (ALL, 2, 128, 64, (6, 5, 7), 2, dict(bias=1)),
    "t_whole": (HALF, 2, 64, 32, (8, 8, 16), 2, dict(bias=1, out=(2, 0))),
    "t_whole_xf": (HALF, 2, 64, 32, (8, 8, 16), 2, dict(bias=1, xf=1, out=(2, 0))),
    "t_odd": (HALF, 2, 64, 31, (4, 8, 8), 2, dict()),
    "acc_igemm": (ALL, 0, 32, 32, (8, 8, 16), 2, dict(acc=1)),
    "acc_ws2": (ALL, 0, 32, 64, (48, 48, 52), 3, dict(acc=1)),
    "flat_s1": (ALL, 0, 32, 64, (72, 80), 2, dict(bias=1, stats=1, flat=1)),
    "flat_s2": (ALL, 1, 32, 64, (48, 80), 2, dict(flat=1)),
    "flat_t": (ALL, 2, 64, 32, (24, 40), 2, dict(bias=1, flat=1)),
}


def _fwd_reference(dtype, mode, cin, cout, size, n, o, seed):
    """operands (storage-rounded, fp32 tensors), the fp64 reference and acc -- CPU only"""
    flat = bool(o.get("flat"))
    taps = 9 if flat else 27
    x = rnd(_mk((n, cin) + size, seed), dtype)
    if mode == 2:
        w = rnd(_mk((cin, cout) + (3,) * len(size), seed + 1) * (cin * taps / 2 ** len(size)) ** -0.5, dtype)
    else:
        w = rnd(_mk((cout, cin) + (3,) * len(size), seed + 1) * (cin * taps) ** -0.5, dtype)
    b = _mk((cout,), seed + 2) if o.get("bias") else None
    op = _torch_conv(mode, flat)
    b64 = b.double() if b is not None else None
    spread, scale, shift = 0.0, None, None
    xa = x
    if o.get("xf"):
        scale, shift = _mk((n, cin), seed + 3) * 0.5 + 1.0, _mk((n, cin), seed + 4) * 0.3
        xa, xb = _operand(x.view((n, cin) + size + (1,) * (3 - len(size))), scale, shift, dtype)
        xa, xb = xa.view(x.shape), xb.view(x.shape)
    ref64, ref32 = op(xa.double(), w.double(), b64), op(xa, w, b)
    if o.get("xf"):
        spread = float((op(xb.double(), w.double(), b64) - ref64).abs().max())
    base = None
    if o.get("acc"):
        base = rnd(_mk(tuple(ref64.shape), seed + 5), dtype)
        ref64, ref32 = ref64 + base.double(), ref32 + base       # RNE(float(existing) + conv)
    return dict(x=x, w=w, b=b, scale=scale, shift=shift, base=base, ref64=ref64, ref32=ref32,
                acc=_acc(ref32, ref64) + spread)


def _as5d(t, flat):
    return t.unsqueeze(2) if flat else t


@pytest.mark.parametrize("case,dtype", [(k, d) for k, v in FWD.items() for d in v[0]],
                         ids=lambda v: v if isinstance(v, str) else NAME[v])
def test_conv_forward(case, dtype):
    _, mode, cin, cout, size, n, o = FWD[case]
    flat = bool(o.get("flat"))
    r = _fwd_reference(dtype, mode, cin, cout, size, n, o, 100)
    xcl = to_cl(_as5d(r["x"], flat), dtype)
    if o.get("in2"):
        wide_in = torch.zeros(xcl.shape[:4] + (2 * cin,), dtype=xcl.dtype, device=DEV)
        wide_in[..., cin:] = xcl
        vin, ipitch = wide_in.view(-1)[cin:], 2 * cin
    else:
        vin, ipitch = xcl.view(-1), cin
    osz = tuple(_as5d(r["ref64"], flat).shape[2:])
    pm, lead = o.get("out", (1, 0))
    wide_out = torch.full((n,) + osz + (pm * cout,), 7.0, dtype=xcl.dtype, device=DEV)
    sl = slice(lead * cout, (lead + 1) * cout)
    if r["base"] is not None:
        wide_out[..., sl] = to_cl(_as5d(r["base"], flat), dtype)
    vout = wide_out.view(-1)[lead * cout:]
    guard = torch.full((64,), 7.0, dtype=xcl.dtype, device=DEV)
    wp = _pack(r["w"], dtype, mode, cin, cout, flat)
    part = None
    if o.get("stats"):
        tiles = lib().hdf_op_conv3d_stat_tiles(dtype, cin, *osz)
        part = torch.zeros((n * tiles, rup(cout, 32), 2), dtype=torch.float32, device=DEV)
    dev = [t.to(DEV).contiguous() if t is not None else None for t in (r["b"], r["scale"], r["shift"])]
    d, h, w_ = xcl.shape[1:4]
    xf = 1 if o.get("xf") else 0
    if o.get("wr"):
        check(lib().hdf_op_conv3d_wr(dtype, ptr(vin), ipitch, cin, n, d, h, w_, ptr(wp), ptr(dev[0]), ptr(dev[1]), ptr(dev[2]),
                                     xf, ptr(vout), pm * cout, cout, ptr(part), 1 if o.get("acc") else 0, st()), "conv3d_wr")
    else:
        check(lib().hdf_op_conv3d(dtype, mode, ptr(vin), ipitch, cin, n, d, h, w_, ptr(wp), ptr(dev[0]), ptr(dev[1]),
                                  ptr(dev[2]), xf, ptr(vout), pm * cout, cout, ptr(part), 1 if o.get("acc") else 0, st()),
              "conv3d")
    torch.cuda.synchronize()
    got = from_cl(wide_out[..., sl])
    got = got[:, :, 0] if flat else got
    _held("conv_forward." + case, dtype, got, r["ref64"], r["acc"])
    if pm > 1:      # the neighbouring channel slices are untouched
        rest = torch.cat([wide_out[..., :lead * cout], wide_out[..., (lead + 1) * cout:]], -1)
        assert bool((rest == 7.0).all())
    assert bool((guard == 7.0).all())
    if part is not None:
        rows = part.view(n, part.shape[0] // n, -1, 2).double().sum(1).cpu()[:, :cout]
        _stats_held("conv_forward." + case, dtype, rows, r["ref32"], r["ref64"], tuple(range(2, r["ref64"].dim())))


@pytest.mark.parametrize("dtype", ALL, ids=NAME.get)
@pytest.mark.parametrize("cin,cout,split,size", [(64, 64, 32, (16, 24, 16)), (32, 64, 32, (48, 48, 48))],
                         ids=["igemm", "ws2"])
def test_conv_split_output(dtype, cin, cout, split, size):
    """hdf_op_conv3d_split: channels [0, split) and [split, Cout) into two dense buffers, the column sums of the first half
    from the statistics rows"""
    n = 2
    r = _fwd_reference(dtype, 0, cin, cout, size, n, {}, 200)
    wp = _pack(r["w"], dtype, 0, cin, cout, False)
    xcl = to_cl(r["x"], dtype)
    o1 = torch.full((n,) + size + (split,), 7.0, dtype=xcl.dtype, device=DEV)
    o2 = torch.full((n,) + size + (cout - split,), 7.0, dtype=xcl.dtype, device=DEV)
    tiles = lib().hdf_op_conv3d_stat_tiles(dtype, cin, *size)
    part = torch.zeros((n * tiles, rup(cout, 32), 2), dtype=torch.float32, device=DEV)
    colsum = torch.zeros(split, dtype=torch.float32, device=DEV)
    check(lib().hdf_op_conv3d_split(dtype, ptr(xcl), cin, cin, n, *size, ptr(wp), ptr(o1), ptr(o2), split, cout, split,
                                    ptr(part), ptr(colsum), split, st()), "conv3d_split")
    torch.cuda.synchronize()
    got = torch.cat([from_cl(o1), from_cl(o2)], 1)
    _held("conv_split", dtype, got, r["ref64"], r["acc"])
    rows = part.view(n, tiles, -1, 2).double().sum(1).cpu()[:, :cout]
    _stats_held("conv_split", dtype, rows, r["ref32"], r["ref64"], (2, 3, 4))
    want = r["ref64"][:, :split].sum((0, 2, 3, 4))
    tol = 4 * float((r["ref32"][:, :split].sum((0, 2, 3, 4)).double() - want).abs().max()) + float(
        (2.0 ** -24 * want.abs()).max())                    # (one more fp32 rounding: the sum is stored as a float)
    assert float((colsum.cpu().double() - want).abs().max()) <= tol


@pytest.mark.parametrize("dtype", HALF, ids=NAME.get)
@pytest.mark.parametrize("cin,cout,size,n", [(4, 32, (8, 16, 24), 2), (1, 16, (4, 8, 16), 3)], ids=["cin4", "cin1"])
@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
def test_conv_first_layer(dtype, cin, cout, size, n, with_bias):
    """hdf_op_conv3d_first (tap-packed K): the weight is the fp32 tensor, rounded to the storage type inside"""
    x = rnd(_mk((n, cin) + size, 300), dtype)
    w32 = _mk((cout, cin, 3, 3, 3), 301) * 0.2
    w = rnd(w32, dtype)
    b = _mk((cout,), 302) * 0.1 if with_bias else None
    ref64 = F.conv3d(x.double(), w.double(), b.double() if with_bias else None, padding=1)
    ref32 = F.conv3d(x, w, b, padding=1)
    xin = torch.full((n,) + size + (16,), 7.0, dtype=TDT[dtype], device=DEV)
    xin[..., :4] = 0
    xin[..., :cin] = x.to(DEV).permute(0, 2, 3, 4, 1).to(TDT[dtype])
    coutp = rup(cout, 32)
    out = torch.full((n,) + size + (coutp,), 7.0, dtype=TDT[dtype], device=DEV)
    part = torch.full((n, 512, coutp, 2), float("nan"), device=DEV)
    wd = w32.to(DEV).contiguous()
    bd = b.to(DEV).contiguous() if with_bias else None
    check(lib().hdf_op_conv3d_first(dtype, ptr(xin), 16, cin, n, *size, ptr(wd), ptr(bd), ptr(out), coutp, cout, ptr(part),
                                    st()), "conv3d_first")
    torch.cuda.synchronize()
    _held("conv_first", dtype, from_cl(out[..., :cout]), ref64, _acc(ref32, ref64))
    assert bool((out[..., cout:] == 7.0).all())
    rows = part.double().sum(1).cpu()
    _stats_held("conv_first", dtype, rows[:, :cout], ref32, ref64, (2, 3, 4))
    assert bool((rows[:, cout:] == 0).all())


# ------------------------------------------------------------------------------------------------ weight gradients
def _wg(op, x, dy, wshape):
    wz = torch.zeros(wshape, dtype=x.dtype, requires_grad=True)
    op(x, wz, None).backward(dy)
    return wz.grad


# name: (dtypes, stride, cin, cout, size (of the SMALL tensor), n, options: xf / acc / pad (Cin stored of 16) / flat)
WGRAD = {
    "s1_small": (ALL, 1, 32, 32, (12, 16, 24), 2, dict()),
    "s1_256_tiles": (ALL, 1, 32, 32, (32, 40, 48), 2, dict()),
    "s1_256_tiles_batch3": (ALL, 1, 64, 32, (21, 48, 50), 3, dict()),
    "s1_accumulate": (ALL, 1, 64, 48, (9, 7, 10), 2, dict(acc=1)),
    "s1_accumulate_256_tiles": (HALF, 1, 32, 32, (32, 40, 48), 2, dict(acc=1)),
    "s1_padded_first_layer": (ALL, 1, 4, 32, (8, 8, 16), 2, dict(pad=1)),
    "t_generic": (ALL, 2, 64, 32, (6, 5, 7), 2, dict()),
    "t_whole": (HALF, 2, 64, 32, (8, 12, 16), 2, dict()),
    "t_whole_xf": (HALF, 2, 128, 64, (16, 16, 16), 3, dict(xf=1)),
    "t_accumulate": (HALF, 2, 32, 32, (20, 8, 12), 2, dict(acc=1)),
    "flat_s1": (ALL, 1, 32, 32, (96, 112), 2, dict(flat=1)),
    "flat_t_xf": (ALL, 2, 64, 32, (24, 40), 2, dict(flat=1, xf=1)),
}


@pytest.mark.parametrize("case,dtype", [(k, d) for k, v in WGRAD.items() for d in v[0]],
                         ids=lambda v: v if isinstance(v, str) else NAME[v])
def test_weight_gradient(case, dtype):
    """hdf_op_conv3d_wgrad: fp32 output from exact products -- no rounding term, every element"""
    _, stride, cin, cout, size, n, o = WGRAD[case]
    flat = bool(o.get("flat"))
    big = tuple(stride * v for v in size)
    x = rnd(_mk((n, cin) + size, 400), dtype)
    dy = rnd(_mk((n, cout) + big, 401), dtype)
    op = _torch_conv(0 if stride == 1 else 2, flat)
    wshape = ((cout, cin) if stride == 1 else (cin, cout)) + (3,) * len(size)
    spread, scale, shift = 0.0, None, None
    xa = x
    if o.get("xf"):      # the transform of the transposed conv's input (the small operand)
        scale = torch.rand(n, cin, generator=torch.Generator().manual_seed(402)) + 0.5
        shift = _mk((n, cin), 403) * 0.3
        xa, xb = _operand(x.view((n, cin) + size + (1,) * (3 - len(size))), scale, shift, dtype)
        xa, xb = xa.view(x.shape), xb.view(x.shape)
    g64, g32 = _wg(op, xa.double(), dy.double(), wshape), _wg(op, xa, dy, wshape)
    if o.get("xf"):
        spread = float((_wg(op, xb.double(), dy.double(), wshape) - g64).abs().max())
    prev = _mk(wshape, 404) if o.get("acc") else None
    if prev is not None:
        g64, g32 = g64 + prev.double(), g32 + prev
    acc = _acc(g32, g64) + spread
    # small / large operand of the launch: stride 1 -> (dy, x); transposed -> (x, dy)
    cp = 16 if o.get("pad") else cin
    x_cl, dy_cl = to_cl(_as5d(x, flat), dtype, cp=cp), to_cl(_as5d(dy, flat), dtype)
    s_cl, sc, l_cl, lc = (dy_cl, cout, x_cl, cp) if stride == 1 else (x_cl, cin, dy_cl, cout)
    dims = s_cl.shape[1:4]
    sc_store, lc_store = wshape[0], wshape[1]
    wsb = lib().hdf_op_wgrad_workspace_bytes(stride, n, *dims, sc, lc)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    if prev is not None:
        p3 = _embed(prev) if flat else prev
        dw = p3.reshape(sc_store, lc_store, 27).to(DEV).contiguous()
    else:
        dw = torch.full((sc_store, lc_store, 27), float("nan"), dtype=torch.float32, device=DEV)
    dev = [t.to(DEV).contiguous() if t is not None else None for t in (scale, shift)]
    check(lib().hdf_op_conv3d_wgrad(dtype, stride, ptr(s_cl), s_cl.shape[-1], sc, ptr(l_cl), l_cl.shape[-1], lc, n, *dims,
                                    ptr(dev[0]), ptr(dev[1]), 1 if o.get("xf") else 0, None, None, 0, ptr(dw), sc_store,
                                    lc_store, 1 if prev is not None else 0, ptr(ws), wsb, st()), "wgrad")
    torch.cuda.synchronize()
    got = dw.cpu().view(sc_store, lc_store, 3, 3, 3)
    if flat:
        assert float(got[:, :, 0].abs().max()) == 0.0 and float(got[:, :, 2].abs().max()) == 0.0
        got = got[:, :, 1]
    _held_sum("wgrad." + case, dtype, got, g64, acc)


def _first_layer_inputs(dtype, cin, size, n):
    x = rnd(_mk((n, cin) + size, 500), dtype)
    xin = torch.full((n,) + size + (16,), 7.0, dtype=TDT[dtype], device=DEV)
    xin[..., :4] = 0
    xin[..., :cin] = x.to(DEV).permute(0, 2, 3, 4, 1).to(TDT[dtype])
    return x, xin


@pytest.mark.parametrize("dtype", HALF, ids=NAME.get)
@pytest.mark.parametrize("cin,cout,size,n", [(4, 32, (8, 16, 24), 2), (1, 16, (5, 9, 11), 3)], ids=["cin4", "cin1"])
@pytest.mark.parametrize("accumulate", [0, 1], ids=["overwrite", "accumulate"])
def test_first_layer_weight_gradient(dtype, cin, cout, size, n, accumulate):
    dy = rnd(_mk((n, cout) + size, 501), dtype)
    x, xin = _first_layer_inputs(dtype, cin, size, n)
    op, wshape = _torch_conv(0, False), (cout, cin, 3, 3, 3)
    g64, g32 = _wg(op, x.double(), dy.double(), wshape), _wg(op, x, dy, wshape)
    prev = _mk(wshape, 502)
    if accumulate:
        g64, g32 = g64 + prev.double(), g32 + prev
    pitch = cout + 16
    dyb = torch.full((n,) + size + (pitch,), 5.0, dtype=TDT[dtype], device=DEV)
    dyb[..., 8:8 + cout] = dy.to(DEV).permute(0, 2, 3, 4, 1).to(TDT[dtype])
    dyv = dyb.view(-1)[8:]
    dw = prev.to(DEV).contiguous() if accumulate else torch.full(wshape, float("nan"), device=DEV)
    ws = torch.empty(64 << 20, dtype=torch.uint8, device=DEV)
    check(lib().hdf_op_conv3d_first_wgrad(dtype, ptr(dyv), pitch, cout, ptr(xin), 16, cin, n, *size, ptr(dw), accumulate,
                                          ptr(ws), ws.numel(), st()), "conv3d_first_wgrad")
    torch.cuda.synchronize()
    _held_sum("first_wgrad", dtype, dw.cpu(), g64, _acc(g32, g64))


def _in_bwd_elem(da, y, sc, sh, mu, rs, k1, ka, kb):
    """hdf_common.h in_bwd_elem in the dtype of the arguments: k1 * ((y*scale+shift > 0 ? da : 0) - ka - (y-mean)*rstd*kb).
    (The sign of y*scale+shift is the same in fp64 and as an fp32 fma: rounding does not cross zero.)"""
    live = y.double() * _bc(sc).double() + _bc(sh).double() > 0
    gg = torch.where(live, da, torch.zeros_like(da))
    return _bc(k1) * (gg - _bc(ka) - (y - _bc(mu)) * _bc(rs) * _bc(kb))


@pytest.mark.parametrize("dtype", HALF, ids=NAME.get)
@pytest.mark.parametrize("cin,cout,size,n", [(4, 32, (8, 16, 24), 2), (2, 64, (5, 9, 11), 3)], ids=["cin4", "cin2"])
def test_first_layer_weight_gradient_norm_inside(dtype, cin, cout, size, n):
    """hdf_op_conv3d_first_wgrad_in: dy by the apply pass of the norm backward, rounded to the storage type, then contracted
    with x.  The rounding of dy can fall either way where fp32 and fp64 disagree: both variants, the spread added to acc."""
    da, y = rnd(_mk((n, cout) + size, 511), dtype), rnd(_mk((n, cout) + size, 512), dtype)
    x, xin = _first_layer_inputs(dtype, cin, size, n)
    vec = [(_mk((n, cout), 513 + i) * 0.3 + (1.0 if i in (0, 3, 4) else 0.0)).contiguous() for i in range(7)]
    dy_a = rnd(_in_bwd_elem(da.double(), y.double(), *[v.double() for v in vec]).float(), dtype)
    dy_b = rnd(_in_bwd_elem(da, y, *vec), dtype)
    op, wshape = _torch_conv(0, False), (cout, cin, 3, 3, 3)
    g64, g32 = _wg(op, x.double(), dy_a.double(), wshape), _wg(op, x, dy_a, wshape)
    acc = _acc(g32, g64) + float((_wg(op, x.double(), dy_b.double(), wshape) - g64).abs().max())
    cl = lambda t: t.to(DEV).permute(0, 2, 3, 4, 1).to(TDT[dtype]).contiguous()
    da_cl, y_cl = cl(da), cl(y)
    dev = [v.to(DEV) for v in vec]
    ws = torch.empty(64 << 20, dtype=torch.uint8, device=DEV)
    got = torch.full(wshape, float("nan"), device=DEV)
    check(lib().hdf_op_conv3d_first_wgrad_in(dtype, ptr(da_cl), cout, cout, ptr(y_cl), cout, *[ptr(v) for v in dev], ptr(xin),
                                             16, cin, n, *size, ptr(got), 0, ptr(ws), ws.numel(), st()), "first_wgrad_in")
    torch.cuda.synchronize()
    _held_sum("first_wgrad_in", dtype, got.cpu(), g64, acc)


def _norm_backward_reference(dtype, n, c, size, seed):
    """relu(InstanceNorm(y) * gamma + beta) backward by the formula of hdf_op_in_bwd (reduce, finalize, apply) in fp64 and in
    fp32: dy = k1 * (g - mean(g) - xhat * mean(g * xhat)), g = da where the activation is positive.  beta is chosen so
    that most activations are positive and gamma varies little: the bias statistic needs 90 % of the elements above 1/64
    of the maximum."""
    y, da = rnd(_mk((n, c) + size, seed), dtype), rnd(_mk((n, c) + size, seed + 1), dtype)
    gamma, beta = _mk((c,), seed + 2) * 0.1 + 1.0, _mk((c,), seed + 3) * 0.2 + 2.5
    mean = y.mean((2, 3, 4))
    rstd = (y.var((2, 3, 4), unbiased=False) + 1e-5).rsqrt()
    scale = (gamma[None] * rstd).contiguous()
    shift = (beta[None] - mean * scale).contiguous()
    out = {}
    for t in (torch.float64, torch.float32):
        yy, dd = y.to(t), da.to(t)
        sc, sh, mu, rs, gm = [v.to(t) for v in (scale, shift, mean, rstd, gamma)]
        live = y.double() * _bc(scale).double() + _bc(shift).double() > 0
        gg = torch.where(live, dd, torch.zeros_like(dd))
        xh = (yy - _bc(mu)) * _bc(rs)
        ka, kb = gg.mean((2, 3, 4)), (gg * xh).mean((2, 3, 4))
        out[t] = (gm[None] * rs)[:, :, None, None, None] * (gg - _bc(ka) - xh * _bc(kb))
    return dict(y=y, da=da, vec=(scale, shift, mean, rstd, gamma), dy64=out[torch.float64], dy32=out[torch.float32])


@pytest.mark.parametrize("dtype", ALL, ids=NAME.get)
@pytest.mark.parametrize("n,c,size", [(2, 32, (8, 12, 16)), (3, 16, (32, 32, 36))], ids=["c32", "c16_large"])
def test_instance_norm_backward(dtype, n, c, size):
    r = _norm_backward_reference(dtype, n, c, size, 600)
    vox = size[0] * size[1] * size[2]
    dy = torch.empty((n,) + size + (c,), dtype=TDT[dtype], device=DEV)
    dg, db = torch.zeros(c, device=DEV), torch.zeros(c, device=DEV)
    ws = torch.empty(lib().hdf_op_in_bwd_workspace_floats(n, c, vox), device=DEV)
    dev = [t.to(DEV).contiguous() for t in r["vec"]]
    da_cl, y_cl = to_cl(r["da"], dtype), to_cl(r["y"], dtype)
    check(lib().hdf_op_in_bwd(dtype, ptr(da_cl), c, ptr(y_cl), c, *[ptr(t) for t in dev], ptr(dy), c, ptr(dg), ptr(db), n, c,
                              vox, ptr(ws), st()), "in_bwd")
    torch.cuda.synchronize()
    _held("in_bwd", dtype, from_cl(dy), r["dy64"], _acc(r["dy32"], r["dy64"]))


@pytest.mark.parametrize("dtype", HALF, ids=NAME.get)
@pytest.mark.parametrize("xf", [False, True], ids=["plain", "xf"])
@pytest.mark.parametrize("n,cin,cout,size", [(2, 32, 32, (16, 16, 24)), (3, 64, 48, (12, 17, 9))], ids=["whole", "ragged"])
def test_norm_backward_inside_weight_gradient(dtype, xf, n, cin, cout, size):
    """hdf_op_in_bwd_wgrad: dy (16-bit, a by-product) to its rounding; dw (fp32) against the fp64 weight gradient of the
    rounded fp64 dy, the spread between the fp64-formed and the fp32-formed dy (and x operand) added to acc"""
    r = _norm_backward_reference(dtype, n, cout, size, 700)
    vox = size[0] * size[1] * size[2]
    x = rnd(_mk((n, cin) + size, 710), dtype)
    xs, xh = (_mk((n, cin), 711) * 0.5 + 1.0, _mk((n, cin), 712) * 0.3) if xf else (None, None)
    xa, xb = _operand(x, xs, xh, dtype) if xf else (x, x)
    dy_a, dy_b = rnd(r["dy64"].float(), dtype), rnd(r["dy32"], dtype)
    op, wshape = _torch_conv(0, False), (cout, cin, 3, 3, 3)
    g64, g32 = _wg(op, xa.double(), dy_a.double(), wshape), _wg(op, xa, dy_a, wshape)
    acc = _acc(g32, g64) + float((_wg(op, xb.double(), dy_b.double(), wshape) - g64).abs().max())
    dev = [t.to(DEV).contiguous() for t in r["vec"]]
    da_cl, y_cl, x_cl = to_cl(r["da"], dtype), to_cl(r["y"], dtype), to_cl(x, dtype)
    xs_d, xh_d = (xs.to(DEV), xh.to(DEV)) if xf else (None, None)
    ws = torch.empty(lib().hdf_op_in_bwd_workspace_floats(n, cout, vox), device=DEV)
    wsb = lib().hdf_op_wgrad_workspace_bytes(1, n, *size, cout, cin)
    wws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    dy = torch.full((n,) + size + (cout,), 7.0, dtype=y_cl.dtype, device=DEV)
    dg, db = torch.zeros(cout, device=DEV), torch.zeros(cout, device=DEV)
    dw = torch.full((cout, cin, 27), float("nan"), dtype=torch.float32, device=DEV)
    check(lib().hdf_op_in_bwd_wgrad(dtype, ptr(da_cl), cout, ptr(y_cl), cout, *[ptr(t) for t in dev], ptr(dy), cout, ptr(dg),
                                    ptr(db), ptr(x_cl), cin, cin, ptr(xs_d), ptr(xh_d), 1 if xf else 0, n, cout, *size,
                                    ptr(dw), ptr(ws), ptr(wws), wsb, st()), "in_bwd_wgrad")
    torch.cuda.synchronize()
    _held("in_bwd_wgrad.dy", dtype, from_cl(dy), r["dy64"], _acc(r["dy32"], r["dy64"]))
    _held_sum("in_bwd_wgrad.dw", dtype, dw.cpu().view(wshape), g64, acc)


@pytest.mark.parametrize("dtype", HALF, ids=NAME.get)
def test_data_gradient_with_norm_backward_rows(dtype):
    """hdf_op_conv3d_bwd_stats: the output to its rounding, and the rows (sum g, sum g * xhat) of the STORED output"""
    cin = cout = 32
    n, size = 2, (48, 48, 56)
    r = _fwd_reference(dtype, 0, cin, cout, size, n, {}, 800)
    y = rnd(_mk((n, cout) + size, 801), dtype)
    sc, sh = _mk((n, cout), 802) * 0.5 + 1.0, _mk((n, cout), 803) * 0.3
    mu, rs = _mk((n, cout), 804) * 0.2, _mk((n, cout), 805).abs() + 0.5
    wp = _pack(r["w"], dtype, 0, cin, cout, False)
    x_cl, y_cl = to_cl(r["x"], dtype), to_cl(y, dtype)
    out = torch.full((n,) + size + (cout,), float("nan"), dtype=x_cl.dtype, device=DEV)
    part = torch.full((n, 512, cout, 2), float("nan"), device=DEV)
    dev = [v.to(DEV).contiguous() for v in (sc, sh, mu, rs)]
    check(lib().hdf_op_conv3d_bwd_stats(dtype, ptr(x_cl), cin, cin, n, *size, ptr(wp), ptr(out), cout, cout, ptr(y_cl), cout,
                                        *[ptr(v) for v in dev], ptr(part), st()), "conv3d_bwd_stats")
    torch.cuda.synchronize()
    got = from_cl(out)
    _held("conv_bwd_stats", dtype, got, r["ref64"], r["acc"])
    # the rows: of `got` itself, so that the check does not depend on the conv's own error; tolerance from the same sums
    # taken in fp32 on the CPU
    live = y.double() * _bc(sc).double() + _bc(sh).double() > 0
    rows = part.double().sum(1).cpu()
    sums = {}
    for t in (torch.float64, torch.float32):
        g = torch.where(live, got.to(t), torch.zeros_like(got, dtype=t))
        xh = (y.to(t) - _bc(mu).to(t)) * _bc(rs).to(t)
        sums[t] = (g.sum((2, 3, 4)).double(), (g * xh).sum((2, 3, 4)).double())
    for k in range(2):
        tol = 4 * float((sums[torch.float32][k] - sums[torch.float64][k]).abs().max())
        err = float((rows[..., k] - sums[torch.float64][k]).abs().max())
        assert err <= tol, (k, err, tol)
        print("ROUNDING conv_bwd_stats.row%d %s %.3f" % (k, NAME[dtype], err / tol))


# ------------------------------------------------------------------------------------------------ elementwise kernels
@pytest.mark.parametrize("dtype", ALL, ids=NAME.get)
def test_norm_relu_add(dtype):
    n, c, size = 2, 32, (8, 12, 16)
    vox = size[0] * size[1] * size[2]
    y, skip = rnd(_mk((n, c) + size, 900), dtype), rnd(_mk((n, c) + size, 901), dtype)
    scale, shift = _mk((n, c), 902) * 0.5 + 1.0, _mk((n, c), 903) * 0.3
    ref64 = torch.relu(y.double() * _bc(scale).double() + _bc(shift).double()) + skip.double()
    ref32 = torch.relu(y * _bc(scale) + _bc(shift)) + skip
    y_cl, sk_cl = to_cl(y, dtype), to_cl(skip, dtype)
    out = torch.empty_like(y_cl)
    sc, sh = scale.to(DEV).contiguous(), shift.to(DEV).contiguous()
    check(lib().hdf_op_norm_relu_add(dtype, ptr(y_cl), c, ptr(sc), ptr(sh), ptr(sk_cl), c, ptr(out), c, n, c, vox, st()),
          "norm_relu_add")
    torch.cuda.synchronize()
    _held("norm_relu_add", dtype, from_cl(out), ref64, _acc(ref32, ref64))


@pytest.mark.parametrize("dtype", ALL, ids=NAME.get)
@pytest.mark.parametrize("c", [32, 48])
def test_encoder_tail(dtype, c):
    n, size = 2, (8, 12, 16)
    y, skip = rnd(_mk((n, c) + size, 910), dtype), rnd(_mk((n, c) + size, 911), dtype)
    scale, shift = _mk((n, c), 912) * 0.5 + 1.0, _mk((n, c), 913) * 0.3
    scale[:, 0] = -scale[:, 0]
    ref64 = torch.relu(y.double() * _bc(scale).double() + _bc(shift).double()) + skip.double()
    ref32 = torch.relu(y * _bc(scale) + _bc(shift)) + skip
    y_cl, sk_cl = to_cl(y, dtype), to_cl(skip, dtype)
    ds = torch.empty_like(y_cl)
    po = torch.empty((n,) + tuple(v // 2 for v in size) + (c,), dtype=y_cl.dtype, device=DEV)
    idx = torch.empty(po.shape, dtype=torch.uint8, device=DEV)
    sc, sh = scale.to(DEV).contiguous(), shift.to(DEV).contiguous()
    check(lib().hdf_op_enc_tail(dtype, ptr(y_cl), c, ptr(sc), ptr(sh), ptr(sk_cl), c, ptr(ds), c, ptr(po), c, ptr(idx), n, c,
                                *po.shape[1:4], st()), "enc_tail")
    torch.cuda.synchronize()
    got = from_cl(ds)
    _held("enc_tail", dtype, got, ref64, _acc(ref32, ref64))
    assert torch.equal(from_cl(po), F.max_pool3d(got, 2))         # the pool of the stored values is exact


def _up(t):
    return F.interpolate(t, scale_factor=2, mode="trilinear", align_corners=False)


@pytest.mark.parametrize("dtype", ALL, ids=NAME.get)
@pytest.mark.parametrize("c,size", [(32, (8, 12, 20)), (16, (2, 2, 2))], ids=["c32", "one_voxel_low"])
def test_encoder_tail_up(dtype, c, size):
    n = 2 if c == 32 else 3
    lo = tuple(v // 2 for v in size)
    y, low = rnd(_mk((n, c) + size, 920), dtype), rnd(_mk((n, c) + lo, 921), dtype)
    scale, shift = _mk((n, c), 922) * 0.5 + 1.0, _mk((n, c), 923) * 0.3
    lscale, lshift = _mk((n, c), 924) * 0.5 + 1.0, _mk((n, c), 925) * 0.3 + 1.0
    d = lambda v: _bc(v).double()
    ref64 = torch.relu(y.double() * d(scale) + d(shift)) + _up(torch.relu(low.double() * d(lscale) + d(lshift)))
    ref32 = torch.relu(y * _bc(scale) + _bc(shift)) + _up(torch.relu(low * _bc(lscale) + _bc(lshift)))
    y_cl, low_cl = to_cl(y, dtype), to_cl(low, dtype)
    ds = torch.empty_like(y_cl)
    po = torch.empty((n,) + lo + (c,), dtype=y_cl.dtype, device=DEV)
    idx = torch.empty(po.shape, dtype=torch.uint8, device=DEV)
    dev = [t.to(DEV).contiguous() for t in (scale, shift, lscale, lshift)]
    check(lib().hdf_op_enc_tail_up(dtype, ptr(y_cl), c, ptr(dev[0]), ptr(dev[1]), ptr(low_cl), c, ptr(dev[2]), ptr(dev[3]),
                                   ptr(ds), c, ptr(po), c, ptr(idx), n, c, *lo, st()), "enc_tail_up")
    torch.cuda.synchronize()
    got = from_cl(ds)
    _held("enc_tail_up", dtype, got, ref64, _acc(ref32, ref64), bias=c == 32)    # (the 2^3 case has 384 elements)
    assert torch.equal(from_cl(po), F.max_pool3d(got, 2))


@pytest.mark.parametrize("dtype", ALL, ids=NAME.get)
@pytest.mark.parametrize("n,c,size", [(2, 32, (8, 12, 16)), (3, 16, (17, 9, 11))], ids=["even", "odd"])
def test_upsample(dtype, n, c, size):
    """hdf_op_upsample_fwd: trilinear x2 of relu(x * scale + shift); hdf_op_upsample_bwd: its adjoint, the gradient read from
    a channel slice of a wider row.  The shift keeps most activations positive (the bias statistic's 90 % condition)."""
    x = rnd(_mk((n, c) + size, 930), dtype)
    scale, shift = _mk((n, c), 931) * 0.3 + 1.0, _mk((n, c), 932) * 0.3 + 1.6
    ref64 = _up(torch.relu(x.double() * _bc(scale).double() + _bc(shift).double()))
    ref32 = _up(torch.relu(x * _bc(scale) + _bc(shift)))
    x_cl = to_cl(x, dtype)
    up = torch.empty((n,) + tuple(2 * s for s in size) + (c,), dtype=x_cl.dtype, device=DEV)
    sc, sh = scale.to(DEV).contiguous(), shift.to(DEV).contiguous()
    check(lib().hdf_op_upsample_fwd(dtype, ptr(x_cl), c, ptr(sc), ptr(sh), ptr(up), c, n, c, *size, st()), "up")
    g = rnd(_mk(tuple(ref64.shape), 933), dtype)
    grads = {}
    for t in (torch.float64, torch.float32):
        leaf = torch.zeros((n, c) + size, dtype=t, requires_grad=True)
        _up(leaf).backward(g.to(t))
        grads[t] = leaf.grad
    gcl = to_cl(g, dtype)
    wide = torch.zeros(gcl.shape[:-1] + (2 * c,), dtype=gcl.dtype, device=DEV)
    wide[..., c:] = gcl
    view = wide.view(-1)[c:]
    dlo = torch.empty_like(x_cl)
    check(lib().hdf_op_upsample_bwd(dtype, ptr(view), 2 * c, ptr(dlo), c, n, c, *size, st()), "upb")
    torch.cuda.synchronize()
    _held("upsample_fwd", dtype, from_cl(up), ref64, _acc(ref32, ref64))
    _held("upsample_bwd", dtype, from_cl(dlo), grads[torch.float64], _acc(grads[torch.float32], grads[torch.float64]))


@pytest.mark.parametrize("dtype", ALL, ids=NAME.get)
def test_maxpool_backward_accumulate(dtype):
    """hdf_op_maxpool_bwd(accumulate=1): din = RNE(float(din) + scatter(dout))"""
    n, c, size = 2, 32, (8, 12, 16)
    ps = tuple(v // 2 for v in size)
    x = rnd(_mk((n, c) + size, 940), dtype)
    x_cl = to_cl(x, dtype)
    po = torch.empty((n,) + ps + (c,), dtype=x_cl.dtype, device=DEV)
    idx = torch.empty(po.shape, dtype=torch.uint8, device=DEV)
    check(lib().hdf_op_maxpool_fwd(dtype, ptr(x_cl), c, ptr(po), c, ptr(idx), n, c, *ps, st()), "pool")
    g, d0 = rnd(_mk((n, c) + ps, 941), dtype), rnd(_mk((n, c) + size, 942), dtype)
    refs = {}
    for t in (torch.float64, torch.float32):
        leaf = x.to(t).requires_grad_(True)
        F.max_pool3d(leaf, 2).backward(g.to(t))
        refs[t] = d0.to(t) + leaf.grad
    din, gcl = to_cl(d0, dtype), to_cl(g, dtype)
    check(lib().hdf_op_maxpool_bwd(dtype, ptr(gcl), c, ptr(idx), ptr(din), c, n, c, *ps, 1, st()), "poolb")
    torch.cuda.synchronize()
    _held("maxpool_bwd_accumulate", dtype, from_cl(din), refs[torch.float64], _acc(refs[torch.float32], refs[torch.float64]))


def _sequential_sum(t):
    """sum over the first axis in the tensor's own precision, one term after the other"""
    s = torch.zeros_like(t[0])
    for row in t:
        s += row
    return s


@pytest.mark.parametrize("dtype", ALL, ids=NAME.get)
@pytest.mark.parametrize("c,ncls,size,n,xf", [(32, 4, (16, 16, 16), 2, True), (64, 3, (8, 12, 16), 3, False),
                                              (48, 6, (9, 7, 15), 2, True)], ids=["c32_xf", "c64", "c48_6cls_xf"])
def test_head(dtype, c, ncls, size, n, xf):
    """hdf_op_head_fwd / _bwd: logits and dx in the storage type, dweight / dbias fp32 (weights and bias are fp32 tensors)"""
    x = rnd(_mk((n, c) + size, 950), dtype)
    w, b = _mk((ncls, c, 1, 1, 1), 951), _mk((ncls,), 952) * 0.1
    w = w / w.pow(2).sum(0, keepdim=True).sqrt() * (ncls / c) ** 0.5     # one scale for every channel of dx (bias statistic)
    scale = torch.rand(n, c, generator=torch.Generator().manual_seed(953)) + 0.5
    shift = _mk((n, c), 954) * 0.3
    dl = rnd(_mk((n, ncls) + size, 955), dtype)
    res = {}
    for t in (torch.float64, torch.float32):
        xt = x.to(t)
        act = (torch.relu(xt * _bc(scale).to(t) + _bc(shift).to(t)) if xf else xt).detach().requires_grad_(True)
        wr, br = w.to(t).requires_grad_(True), b.to(t).requires_grad_(True)
        out = F.conv3d(act, wr, br)
        out.backward(dl.to(t))
        res[t] = (out.detach(), act.grad, wr.grad.view(ncls, c), br.grad, act.detach())
    r64, r32 = res[torch.float64], res[torch.float32]
    vox = size[0] * size[1] * size[2]
    xcl = to_cl(x, dtype)
    logits = torch.empty((n, ncls) + size, dtype=TDT[dtype], device=DEV)
    sc, sh = (scale.to(DEV), shift.to(DEV)) if xf else (None, None)
    wd, bd = w.to(DEV).contiguous(), b.to(DEV)
    check(lib().hdf_op_head_fwd(dtype, ptr(xcl), c, ptr(sc), ptr(sh), ptr(wd), ptr(bd), ptr(logits), n, c, ncls, vox, st()),
          "head_fwd")
    dx = torch.zeros((n,) + size + (c,), dtype=TDT[dtype], device=DEV)
    dw, db = torch.zeros(ncls, c, device=DEV), torch.zeros(ncls, device=DEV)
    dld = dl.to(TDT[dtype]).to(DEV).contiguous()
    check(lib().hdf_op_head_bwd(dtype, ptr(dld), ptr(xcl), c, ptr(sc), ptr(sh), ptr(wd), ptr(dx), c, 0, ptr(dw), ptr(db), n,
                                c, ncls, vox, st()), "head_bwd")
    torch.cuda.synchronize()
    _held("head_fwd.logits", dtype, logits.float().cpu(), r64[0], _acc(r32[0], r64[0]))
    _held("head_bwd.dx", dtype, from_cl(dx), r64[1], _acc(r32[1], r64[1]))
    # dweight / dbias: torch's own fp32 reduction of these 8- and 11-bit summands is exact or nearly so (blocked, pairwise),
    # which would leave no allowance at all; "the same formula in fp32" is taken literally instead, term after term
    rows_dl = dl.permute(0, 2, 3, 4, 1).reshape(-1, ncls)
    rows_act = res[torch.float32][4].permute(0, 2, 3, 4, 1).reshape(-1, c)
    _held_sum("head_bwd.dw", dtype, dw.cpu(), r64[2], _acc(_sequential_sum(rows_dl[:, :, None] * rows_act[:, None, :]), r64[2]))
    _held_sum("head_bwd.db", dtype, db.cpu(), r64[3], _acc(_sequential_sum(rows_dl), r64[3]))


@pytest.mark.parametrize("dtype", HALF, ids=NAME.get)
@pytest.mark.parametrize("DM,N,B,M", [(128, 27, 2, 2), (64, 512, 1, 2)], ids=["dm128_n27", "dm64_n512"])
def test_block_out_attnall(dtype, DM, N, B, M):
    """hdf_op_block_out_fwd writing attnall: DenseForward(DM+128 -> 64 -> DM) in fp32 (eval mode), ONE rounding to the storage
    type into the channels-last [B][N][M*DM] tensor"""
    DMF, rows = DM + 128, B * N
    g = torch.Generator().manual_seed(960 + DM)
    P = [torch.randn(M, 64, DMF, generator=g) * DMF ** -0.5, torch.randn(M, 64, generator=g) * 0.1,
         torch.randn(M, DM, 64, generator=g) * 0.125, torch.randn(M, DM, generator=g) * 0.1]
    Fin = torch.randn(M * rows, DMF, generator=g)
    outs = {}
    for t in (torch.float64, torch.float32):
        o = [F.linear(F.gelu(F.linear(Fin[m * rows:(m + 1) * rows].to(t), P[0][m].to(t), P[1][m].to(t))), P[2][m].to(t),
                      P[3][m].to(t)) for m in range(M)]
        outs[t] = torch.stack(o, 0)                       # [M, rows, DM]
    sizes = [p[0].numel() for p in P]
    offs = [0]
    for s in sizes:
        offs.append(offs[-1] + (s + 15) // 16 * 16)
    mstride = offs[-1]
    flat = torch.zeros(M * mstride)
    for m in range(M):
        for p, o, s in zip(P, offs, sizes):
            flat[m * mstride + o: m * mstride + o + s] = p[m].flatten()
    flat = flat.to(DEV)
    pp = (C.c_void_p * 4)(*[flat[o:].data_ptr() for o in offs[:-1]])
    Fd = Fin.to(DEV)
    attnall = torch.zeros(B, N, M * DM, dtype=TDT[dtype], device=DEV)
    check(lib().hdf_op_block_out_fwd(M, B, N, DM, 1, pp, mstride, ptr(Fd), None, ptr(attnall), dtype, 0, 0, st()),
          "block_out_fwd")
    torch.cuda.synchronize()
    got = attnall.float().cpu().view(B, N, M, DM).permute(2, 0, 1, 3).reshape(M, rows, DM)
    _held("block_out.attnall", dtype, got, outs[torch.float64], _acc(outs[torch.float32], outs[torch.float64]))
