"""The reference side of test_gpu_pool2d_rounding.py, CPU only: the 2-D pooling / up-sampling passes of the 2-D model
(models/HDenseFormer_2D.py:166-170 bilinear x2, align_corners=False; :194-202 MaxPool2d(2)) and the InstanceNorm
statistics' finalize, each restated in plain torch in whatever float type it is asked for (fp64: the reference; fp32: the
accumulation allowance), the data of every case, and the checks.  tests/test_pool2d_ref_cpu.py runs the checks here
against torch emulations of the kernels and of the defects the checks are there to reject.

Tensors are [N, C, H, W] fp32 on the CPU, already rounded through the storage type (hip_util.rnd); scale / shift / mean /
rstd are [N, C] fp32.  Allowance: acc = 4 x max|op in torch fp32 - op in torch fp64| on the same operands (acc_of), a
property of the reference alone.

The finalize (hdf_op_in_finalize) from fp32 partial rows [N][tiles][CP][2] = per-tile (sum, sum of squares), with the sums
over the tiles in fp64:  m = S1 / vox;  var = max(S2 / vox - m^2, 0);  r = 1 / sqrt(var + eps);  scale = gamma r;
shift = beta - m gamma r  (gamma = 1, beta = 0 where not given).  eps is the fp32 value the entry takes (its argument is
a float): an operand like any other.  Bounds, with q evaluated with the tiles summed forward and reversed and
ord(q) = 4 |q_fwd - q_rev| + 2^-50 |q|:
    mean, rstd   |got - q| <= 0.5 ulp_fp32(q) + ord(q)
    scale        <= 1.001 * 2^-23 |gamma r| + |gamma| ord(r)                               (two fp32 roundings)
    shift        <= 3 * 2^-23 (|beta| + |m gamma r|) + |gamma| (|m| ord(r) + |r| ord(m))   (the fp32 roundings of m, r, two
                 products and the subtraction, with or without contraction)
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from hdf_rt._lib import BF16, F16, F32
from hip_util import check_rounded, check_rounding_bias, rnd, ulp_of

NAME = {F32: "f32", BF16: "bf16", F16: "f16"}
ALL = [F32, BF16, F16]
GUARD = 64            # elements of 7.0 behind every output tensor

# (N, C, pooled Ho, pooled Wo): bias statistic yes / no
ENC_TAIL = {"base": (2, 32, 12, 20, True), "c48_odd": (2, 48, 9, 13, True), "one_window": (3, 16, 1, 1, False)}
# (N, C, Hi, Wi): bias statistic yes / no
UPSAMPLE = {"base": (2, 32, 24, 40, True), "odd": (3, 16, 17, 23, True), "gx2_slab": (2, 64, 12, 40, True),
            "h1": (2, 16, 1, 9, False), "w1": (2, 16, 9, 1, False)}
# (N, C, pooled Ho, pooled Wo): rows per sample
POOL_BWD = {"rows4": (2, 32, 25, 41, 4), "lanes21": (2, 48, 19, 25, 2), "row1": (3, 16, 6, 10, 1)}
# the case of each family whose operands are channel slices of a 2C row
PITCHED = {"enc_tail": "c48_odd", "upsample": "odd", "pool_bwd": "lanes21"}


def mk(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def bc(v):
    return v[:, :, None, None]


def acc_of(ref32, ref64, factor=4.0):
    """the accumulation allowance: a property of the reference alone"""
    return factor * float((ref32.double() - ref64).abs().max())


# ------------------------------------------------------------------------------------------------ the operations
def act(x, scale, shift, t):
    return torch.relu(x.to(t) * bc(scale).to(t) + bc(shift).to(t))


def enc_tail(y, scale, shift, skip, t):
    """ds = relu(y * scale + shift) + skip"""
    return act(y, scale, shift, t) + skip.to(t)


def window_pos(stored):
    """MaxPool2d(2) of the STORED values: (pooled, position of the maximum in its window as 2 dy + dx).  torch keeps the
    first maximum in scan order (h, then w), the kernel's strict >."""
    pooled, flat = F.max_pool2d(stored, 2, return_indices=True)
    w = stored.shape[-1]
    return pooled, (2 * ((flat // w) % 2) + (flat % w) % 2).to(torch.uint8)


def up2(t):
    return F.interpolate(t, scale_factor=2, mode="bilinear", align_corners=False)


def upsample(x, scale, shift, t):
    return up2(act(x, scale, shift, t))


def up2_adjoint(g, t):
    """the adjoint of the bilinear x2, by autograd"""
    leaf = torch.zeros(g.shape[:2] + (g.shape[2] // 2, g.shape[3] // 2), dtype=t, requires_grad=True)
    up2(leaf).backward(g.to(t))
    return leaf.grad


def pool_backward(stored, g, d0, t):
    """d0 + MaxPool2d(2) backward of g at the maxima of the stored tensor"""
    leaf = stored.detach().to(t, copy=True).requires_grad_(True)
    F.max_pool2d(leaf, 2).backward(g.to(t))
    return d0.to(t) + leaf.grad


def rows_per_sample(c, pvox):
    """hdf_op_maxpool_bwd_in_rows(C, 1, Ho, Wo) (include/hdf.h); the GPU test compares it with the library's answer"""
    return max(1, min(1024, pvox * (c // 4) // 2048))


def first_pass(din, y, scale, shift, mean, rstd):
    """the first pass of the InstanceNorm(+ReLU) backward on the stored gradient din: per (n, c) the sums
    (sum g, sum g * (y - mean) * rstd), g = din where y * scale + shift > 0.  Returns (want [N, C, 2] fp64, tol [N, C, 2],
    flipped): tol = 4 x the largest fp32-vs-fp64 difference of the same sums, plus, per (n, c), |g| resp. |g xhat| of every
    element whose mask differs between the fp64 evaluation (what an fma gives) and the unfused fp32 one; flipped = the
    fraction of such elements."""
    m64 = y.double() * bc(scale).double() + bc(shift).double() > 0
    m32 = y * bc(scale) + bc(shift) > 0
    sums = {}
    for t in (torch.float64, torch.float32):
        g = torch.where(m64, din.to(t), torch.zeros_like(din, dtype=t))
        xh = (y.to(t) - bc(mean).to(t)) * bc(rstd).to(t)
        sums[t] = torch.stack([g.sum((2, 3)), (g * xh).sum((2, 3))], -1).double()
    want = sums[torch.float64]
    spread = (sums[torch.float32] - want).abs().amax((0, 1))                       # [2]
    flip = (m64 != m32).double()
    xh = (y.double() - bc(mean).double()) * bc(rstd).double()
    extra = torch.stack([(flip * din.double().abs()).sum((2, 3)), (flip * (din.double() * xh).abs()).sum((2, 3))], -1)
    return want, 4 * spread[None, None, :] + extra, float(flip.mean())


def check_rows(case, dtype, rows64, din, y, scale, shift, mean, rstd):
    """rows64 [N, C, 2]: the partial rows summed in fp64 over the rows of a sample; din: the RETURNED gradient"""
    assert bool(torch.isfinite(rows64).all()), "%s: a partial row was not written" % case
    want, tol, _ = first_pass(din, y, scale, shift, mean, rstd)
    err = (rows64 - want).abs()
    for k in range(2):
        worst = float((err[..., k] / tol[..., k].clamp_min(1e-300)).max())
        print("ROUNDING %s.row%d %s %.3f" % (case, k, NAME[dtype], worst))
    bad = err > tol
    assert not bool(bad.any()), "%s: row sums of (n, c, k) %s off by %.3e, allowed %.3e" % (
        case, tuple(int(v) for v in torch.unravel_index((err / tol.clamp_min(1e-300)).argmax(), err.shape)),
        float(err[bad].max()), float(tol[bad].min()))


# ------------------------------------------------------------------------------------------------ the data of the cases
@functools.lru_cache(maxsize=None)
def enc_tail_case(dtype, n, c, ho, wo, seed=1100):
    """operands and references of hdf_op_enc_tail_2d.  Channel 0: non-negative y, a negative scale and shift and a zero skip,
    so that ds is 0 throughout and every window a tie.  The other channels: a skip around +1 and scales close to 1, which
    keeps 92 % of |ds| at or above max / 64 with the zero channel counted (the bias statistic's condition)"""
    h, w = 2 * ho, 2 * wo
    y, skip = mk((n, c, h, w), seed), mk((n, c, h, w), seed + 1) + 1.0
    scale, shift = mk((n, c), seed + 2) * 0.2 + 1.0, mk((n, c), seed + 3) * 0.3
    y[:, 0], skip[:, 0] = y[:, 0].abs(), 0.0
    scale[:, 0], shift[:, 0] = -scale[:, 0].abs(), -shift[:, 0].abs()
    y, skip = rnd(y, dtype), rnd(skip, dtype)
    ref64, ref32 = enc_tail(y, scale, shift, skip, torch.float64), enc_tail(y, scale, shift, skip, torch.float32)
    assert float(ref64[:, 0].abs().max()) == 0.0
    return dict(y=y, skip=skip, scale=scale, shift=shift, ref64=ref64, ref32=ref32, acc=acc_of(ref32, ref64))


@functools.lru_cache(maxsize=None)
def upsample_case(dtype, n, c, hi, wi, seed=1200):
    """operands and references of hdf_op_upsample_fwd_2d and of hdf_op_upsample_bwd_2d (g: the gradient of the output).
    The shift keeps most activations positive (the bias statistic's 90 % condition)."""
    x = rnd(mk((n, c, hi, wi), seed), dtype)
    scale, shift = mk((n, c), seed + 1) * 0.3 + 1.0, mk((n, c), seed + 2) * 0.3 + 1.6
    ref64, ref32 = upsample(x, scale, shift, torch.float64), upsample(x, scale, shift, torch.float32)
    g = rnd(mk((n, c, 2 * hi, 2 * wi), seed + 3), dtype)
    adj64, adj32 = up2_adjoint(g, torch.float64), up2_adjoint(g, torch.float32)
    return dict(x=x, scale=scale, shift=shift, ref64=ref64, ref32=ref32, acc=acc_of(ref32, ref64), g=g, adj64=adj64,
                adj32=adj32, adj_acc=acc_of(adj32, adj64))


@functools.lru_cache(maxsize=None)
def pool_bwd_case(dtype, n, c, ho, wo, seed=1300):
    """operands of hdf_op_maxpool_bwd_in_2d: the encoder tail's operands (idx and the stored ds come from it), the pooled
    gradient g, the gradient d0 already in din, and the statistics of the layer"""
    r = dict(enc_tail_case(dtype, n, c, ho, wo, seed))
    r["g"], r["d0"] = rnd(mk((n, c, ho, wo), seed + 10), dtype), rnd(mk((n, c, 2 * ho, 2 * wo), seed + 11), dtype)
    r["mean"], r["rstd"] = mk((n, c), seed + 12) * 0.2, mk((n, c), seed + 13).abs() + 0.5
    return r


def pool_bwd_reference(r, stored):
    """din = d0 + scatter(g) at the maxima of `stored` (the encoder tail's stored ds): (fp64, acc)"""
    d64 = pool_backward(stored, r["g"], r["d0"], torch.float64)
    return d64, acc_of(pool_backward(stored, r["g"], r["d0"], torch.float32), d64)


# ------------------------------------------------------------------------------------------------ the checks
def held(case, dtype, got, ref64, acc, bias=True):
    """test_gpu_ops_rounding._held: every element within 0.5 ulp of the storage type + acc of the fp64 reference, then the
    signed bias of the 16-bit roundings"""
    worst = check_rounded(got, ref64, dtype, acc, case)
    if bias and dtype != F32:
        check_rounding_bias(got, ref64, dtype, case)
    print("ROUNDING %s %s %.3f" % (case, NAME[dtype], worst))


def check_enc_tail(case, dtype, r, ds, pooled, idx, bias):
    """ds to the fp64 reference; pooled and idx exactly MaxPool2d(2) of the RETURNED ds, idx = 2 dy + dx of the first
    maximum, 0 throughout the all-tie channel"""
    held(case + ".ds", dtype, ds, r["ref64"], r["acc"], bias)
    want, pos = window_pos(ds)
    assert torch.equal(pooled, want), "%s: pooled is not the maximum of the stored ds" % case
    assert int(idx.max()) < 4, "%s: a window index above 3" % case
    assert torch.equal(idx, pos), "%s: %d window indices differ from torch's" % (case, int((idx != pos).sum()))
    assert int(idx[:, 0].max()) == 0, "%s: a tie did not keep the first maximum" % case


def check_pool_bwd(case, dtype, r, stored, din, rows64, bias=True):
    d64, acc = pool_bwd_reference(r, stored)
    held(case + ".din", dtype, din, d64, acc, bias)
    check_rows(case, dtype, rows64, din, r["y"], r["scale"], r["shift"], r["mean"], r["rstd"])


# ------------------------------------------------------------------------------------------------ the finalize
EPS = 1e-5
FIN_TILES = [1, 31, 33, 128, 129, 515]
FIN_CHANNELS = [(32, 32), (48, 64), (63, 64)]
FIN_N, FIN_TILE_VOX = 2, 512
CONST_CHANNEL = (0, 5, 1.375)       # (sample, channel, value): var = 0 exactly, rstd = 1 / sqrt(eps)
# a second constant channel whose fp32 sum of squares rounds BELOW vox * value^2: S2 / vox - m^2 < 0 before the clamp
NEG_VAR_CHANNEL = (1, 7, 1.1)


@functools.lru_cache(maxsize=None)
def finalize_partials(tiles, c, cp, seed=1400):
    """[N][tiles][CP][2] fp32 (numpy): per-tile (sum, sum of squares), rounded to fp32, of 512 values drawn per (n, c) with
    a mean in {0.1, 1, 10} x N(0, 1) and a standard deviation in {0.05, 1, 3}; channels C..CP-1 are NaN"""
    rng = np.random.default_rng(seed + 7 * tiles + cp + c)
    part = np.full((FIN_N, tiles, cp, 2), np.nan, dtype=np.float32)
    for n in range(FIN_N):
        mean = rng.choice([0.1, 1.0, 10.0], size=c) * rng.standard_normal(c)
        std = rng.choice([0.05, 1.0, 3.0], size=c)
        v = rng.standard_normal((tiles, FIN_TILE_VOX, c), dtype=np.float32).astype(np.float64) * std + mean
        for nn, ch, val in (CONST_CHANNEL, NEG_VAR_CHANNEL):
            if nn == n:
                v[:, :, ch] = np.float64(np.float32(val))
        part[n, :, :c, 0] = v.sum(1).astype(np.float32)
        part[n, :, :c, 1] = (v * v).sum(1).astype(np.float32)
    return part


@functools.lru_cache(maxsize=None)
def finalize_affine(c, seed=1450):
    rng = np.random.default_rng(seed + c)
    return (rng.standard_normal(c) * 0.3 + 1.0).astype(np.float32), (rng.standard_normal(c) * 0.3).astype(np.float32)


def finalize(part, c, vox, gamma, beta, eps, reverse=False):
    """(m, r, scale, shift), each [N, C] fp64, from partials [N][tiles][CP][2]; the tiles summed one after the other in
    fp64, last first if reverse"""
    p = part[:, ::-1] if reverse else part
    s = np.zeros((part.shape[0], c, 2))
    for t in range(p.shape[1]):
        s += p[:, t, :c].astype(np.float64)
    m = s[..., 0] / vox
    var = np.maximum(s[..., 1] / vox - m * m, 0.0)
    r = 1.0 / np.sqrt(var + np.float64(np.float32(eps)))
    g = np.ones(c) if gamma is None else gamma.astype(np.float64)
    b = np.zeros(c) if beta is None else beta.astype(np.float64)
    return m, r, g[None] * r, b[None] - m * g[None] * r


def _ulp32(q):
    return ulp_of(torch.from_numpy(np.ascontiguousarray(q)), F32).numpy()


def finalize_bounds(part, c, vox, gamma, beta, eps):
    """{name: (reference, bound)} per the module docstring"""
    fwd, rev = finalize(part, c, vox, gamma, beta, eps), finalize(part, c, vox, gamma, beta, eps, reverse=True)
    m, r, sc, sh = fwd
    om = 4 * np.abs(m - rev[0]) + 2.0 ** -50 * np.abs(m)
    orr = 4 * np.abs(r - rev[1]) + 2.0 ** -50 * np.abs(r)
    g = np.ones(c) if gamma is None else np.abs(gamma.astype(np.float64))
    b = np.zeros(c) if beta is None else np.abs(beta.astype(np.float64))
    return {"mean": (m, 0.5 * _ulp32(m) + om), "rstd": (r, 0.5 * _ulp32(r) + orr),
            "scale": (sc, 1.001 * 2.0 ** -23 * np.abs(sc) + g[None] * orr),
            "shift": (sh, 3 * 2.0 ** -23 * (b[None] + np.abs(m * sc)) + g[None] * (np.abs(m) * orr + np.abs(r) * om))}


def check_finalize(case, got, part, c, vox, gamma, beta, eps=EPS):
    """got: {mean, rstd, scale, shift} -> [N, C] arrays (fp32).  Every element within its bound (a NaN fails); returns the
    worst error / bound per output."""
    worst = {}
    for name, (ref, bound) in finalize_bounds(part, c, vox, gamma, beta, eps).items():
        err = np.abs(np.asarray(got[name], dtype=np.float64) - ref)
        ratio = err / np.maximum(bound, 1e-300)
        worst[name] = float(np.max(np.where(np.isnan(ratio), np.inf, ratio)))
        print("ROUNDING %s.%s %.3f" % (case, name, worst[name]))
    for name, w in worst.items():
        assert w <= 1.0, "%s: %s is %.3f x its bound" % (case, name, w)
    n, ch, _ = CONST_CHANNEL
    if ch < c:      # the clamp holds: the constant channel's rstd is 1 / sqrt(eps) = 316.2278
        ref = 1.0 / np.sqrt(np.float64(np.float32(eps)))
        assert abs(float(got["rstd"][n, ch]) - ref) <= 0.5 * float(_ulp32(np.array([ref]))[0]) + 2.0 ** -50 * ref
    return worst
