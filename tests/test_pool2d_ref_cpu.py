"""CPU self-tests of tests/pool2d_ref.py: torch emulations of the 2-D pooling / up-sampling kernels (csrc/pool_ops.hip,
FLAT forms) and of in_finalize_kernel (csrc/norm_ops.hip) pass the checks of test_gpu_pool2d_rounding.py on the data of
its cases, the conditions on that data hold (bias statistic: 90 % of the elements at or above max / 64 and 10 000 of them;
fewer than 1 in 1000 activation masks that differ between fp32 and fp64), and every planted defect fails the check that is
there for it -- each on the smallest case that has the feature."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pool2d_ref as R
from hdf_rt._lib import BF16, F16, F32
from hip_util import rnd, signed_rounding_bias

HALF = [BF16, F16]
IDS = R.NAME.get


def _truncate(r32, dtype):
    """fp32 -> storage type by dropping the low bits (round toward zero), returned as fp32"""
    mask = ~0xFFFF if dtype == BF16 else ~0x1FFF
    return (r32.contiguous().view(torch.int32) & mask).view(torch.float32)


def _store(f32, dtype, trunc=False):
    return _truncate(f32, dtype) if trunc else rnd(f32, dtype)


# ------------------------------------------------------------------------------------------------ emulations (fp32)
def emu_enc_tail(r, dtype, trunc=False, transposed_index=False, keep_last=False):
    ds = _store(torch.relu(r["y"] * R.bc(r["scale"]) + R.bc(r["shift"])) + r["skip"], dtype, trunc)
    best = torch.full_like(ds[:, :, ::2, ::2], float("-inf"))
    bi = torch.zeros(best.shape, dtype=torch.uint8)
    for k in range(4):
        dy, dx = k >> 1, k & 1
        v = ds[:, :, dy::2, dx::2]
        upd = v >= best if keep_last else v > best
        best = torch.where(upd, v, best)
        bi = torch.where(upd, torch.full_like(bi, 2 * dx + dy if transposed_index else k), bi)
    return ds, best, bi


def _up_axis(L, dim, zero_pad, swap):
    n = L.shape[dim]
    i = torch.arange(n)
    prev, nxt = L.index_select(dim, (i - 1).clamp_min(0)), L.index_select(dim, (i + 1).clamp_max(n - 1))
    if zero_pad:
        prev, nxt = prev.clone(), nxt.clone()
        prev.select(dim, 0).zero_()
        nxt.select(dim, n - 1).zero_()
    a, b = (0.75, 0.25) if swap else (0.25, 0.75)
    return torch.stack([a * prev + b * L, b * L + a * nxt], dim + 1).flatten(dim, dim + 1)


def emu_upsample(r, dtype, trunc=False, zero_pad=False, swap=False):
    L = torch.relu(r["x"] * R.bc(r["scale"]) + R.bc(r["shift"]))
    return _store(_up_axis(_up_axis(L, 3, zero_pad, swap), 2, zero_pad, swap), dtype, trunc)


def _adj_axis(G, dim, drop_border):
    """up_bwd_taps: input i receives .25 of output 2i-1, .75 of 2i and 2i+1 (1.0 at the clamped ends), .25 of 2i+2"""
    n = G.shape[dim] // 2
    ev, od = G.unflatten(dim, (n, 2)).select(dim + 1, 0), G.unflatten(dim, (n, 2)).select(dim + 1, 1)
    shape = [1] * ev.dim()
    shape[dim] = n
    w1, w2 = torch.full((n,), 0.75), torch.full((n,), 0.75)
    w1[0] = 1.0
    w2[n - 1] = 0.75 if drop_border else 1.0
    out = w1.view(shape) * ev + w2.view(shape) * od
    out.narrow(dim, 1, n - 1).add_(0.25 * od.narrow(dim, 0, n - 1))
    out.narrow(dim, 0, n - 1).add_(0.25 * ev.narrow(dim, 1, n - 1))
    return out


def emu_adjoint(r, dtype, trunc=False, drop_border=False):
    return _store(_adj_axis(_adj_axis(r["g"], 3, False), 2, drop_border), dtype, trunc)


def emu_pool_bwd(r, idx, dtype, trunc=False, without_old=False, skip_last_row=False):
    """(din, rows [N, rows, C, 2] fp32): the scatter, then per row the thread's running sums over its pooled voxels (4 window
    elements each, lane-strided) and the lanes one after the other, all in fp32"""
    din = torch.zeros_like(r["d0"]) if without_old else r["d0"].clone()
    for k in range(4):
        din[:, :, k >> 1::2, k & 1::2] += torch.where(idx == k, r["g"], torch.zeros_like(r["g"]))
    din = _store(din, dtype, trunc)
    n, c, h, w = din.shape
    pvox = (h // 2) * (w // 2)
    blocks, vlanes = R.rows_per_sample(c, pvox), 256 // (c // 4)
    per = -(-pvox // blocks)
    steps = -(-per // vlanes)
    y = r["y"]
    live = y.double() * R.bc(r["scale"]).double() + R.bc(r["shift"]).double() > 0        # (the kernel's fma)
    g = torch.where(live, din, torch.zeros_like(din))
    rows = torch.zeros(n, blocks, c, 2)
    for k, t in enumerate((g, g * ((y - R.bc(r["mean"])) * R.bc(r["rstd"])))):
        win = t.view(n, c, h // 2, 2, w // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(n, c, pvox, 4)
        win = F.pad(win, (0, 0, 0, blocks * per - pvox)).view(n, c, blocks, per, 4)
        win = F.pad(win, (0, 0, 0, steps * vlanes - per)).view(n, c, blocks, steps, vlanes, 4)
        s = torch.zeros(n, c, blocks, vlanes)
        for j in range(steps):
            for q in range(4):
                s = s + win[:, :, :, j, :, q]
        tot = torch.zeros(n, c, blocks)
        for lane in range(vlanes):
            tot = tot + s[..., lane]
        rows[..., k] = tot.permute(0, 2, 1)
    if skip_last_row:
        rows[:, -1] = 0
    return din, rows


def emu_finalize(part, c, cp, vox, gamma, beta, eps=R.EPS, unbiased=False, clamp=True, remainder=True, pitch=None):
    """in_finalize_kernel: 32 tile lanes, 4 loads per pass then one by one, fp64; the lanes one after the other; mean and
    rstd rounded to fp32, scale and shift in fp32"""
    n_, tiles = part.shape[:2]
    pitch = pitch or cp
    flat = part.reshape(-1)
    ch = np.arange(c)

    def rd(t):      # [N, C, 2] of tile t
        base = ((np.arange(n_)[:, None] * tiles + t) * pitch + ch[None, :]) * 2
        return np.stack([flat[base], flat[base + 1]], -1).astype(np.float64)

    s = np.zeros((n_, c, 2))
    for lane in range(32):
        a = np.zeros((n_, c, 2))
        t = lane
        while t + 96 < tiles:
            a += (rd(t) + rd(t + 32)) + (rd(t + 64) + rd(t + 96))
            t += 128
        while remainder and t < tiles:
            a += rd(t)
            t += 32
        s = a if lane == 0 else s + a
    m = s[..., 0] / vox
    var = s[..., 1] / vox - m * m
    if unbiased:
        var = var * vox / (vox - 1)
    if clamp:
        var = np.maximum(var, 0.0)
    with np.errstate(invalid="ignore"):
        r = (1.0 / np.sqrt(var + np.float64(np.float32(eps)))).astype(np.float32)
    g = np.ones(c, np.float32) if gamma is None else gamma
    b = np.zeros(c, np.float32) if beta is None else beta
    m32 = m.astype(np.float32)
    return dict(mean=m32, rstd=r, scale=g[None] * r, shift=b[None] - m32 * g[None] * r)


# ------------------------------------------------------------------------------------------------ the emulations pass
def _bias_conditions(got, ref64, dtype, what):
    if dtype != F32:
        _, used, total = signed_rounding_bias(got, ref64, dtype)
        print("FRACTION %s %s %.3f of %d" % (what, R.NAME[dtype], used / total, total))
        assert used >= 0.9 * total and used >= 10000, (what, used, total)


@pytest.mark.parametrize("dtype", R.ALL, ids=IDS)
@pytest.mark.parametrize("case", list(R.ENC_TAIL))
def test_encoder_tail_emulation_passes(case, dtype):
    n, c, ho, wo, bias = R.ENC_TAIL[case]
    r = R.enc_tail_case(dtype, n, c, ho, wo)
    ds, pooled, idx = emu_enc_tail(r, dtype)
    if bias:
        _bias_conditions(ds, r["ref64"], dtype, "enc_tail." + case)
    R.check_enc_tail("enc_tail_2d." + case, dtype, r, ds, pooled, idx, bias)


@pytest.mark.parametrize("dtype", R.ALL, ids=IDS)
@pytest.mark.parametrize("case", list(R.UPSAMPLE))
def test_upsample_emulations_pass(case, dtype):
    n, c, hi, wi, bias = R.UPSAMPLE[case]
    r = R.upsample_case(dtype, n, c, hi, wi)
    up, adj = emu_upsample(r, dtype), emu_adjoint(r, dtype)
    assert float((r["ref64"] > 0).double().mean()) >= 0.9
    if bias:
        _bias_conditions(up, r["ref64"], dtype, "upsample_fwd." + case)
        _bias_conditions(adj, r["adj64"], dtype, "upsample_bwd." + case)
    R.held("upsample_fwd_2d." + case, dtype, up, r["ref64"], r["acc"], bias)
    R.held("upsample_bwd_2d." + case, dtype, adj, r["adj64"], r["adj_acc"], bias)


@pytest.mark.parametrize("dtype", R.ALL, ids=IDS)
@pytest.mark.parametrize("case", list(R.POOL_BWD))
def test_pool_backward_emulation_passes(case, dtype):
    n, c, ho, wo, nrows = R.POOL_BWD[case]
    assert R.rows_per_sample(c, ho * wo) == nrows
    r = R.pool_bwd_case(dtype, n, c, ho, wo)
    stored, _, idx = emu_enc_tail(r, dtype)
    din, rows = emu_pool_bwd(r, idx, dtype)
    _bias_conditions(din, R.pool_bwd_reference(r, stored)[0], dtype, "pool_bwd." + case)
    flipped = R.first_pass(din, r["y"], r["scale"], r["shift"], r["mean"], r["rstd"])[2]
    assert flipped < 1e-3, flipped
    R.check_pool_bwd("maxpool_bwd_in_2d." + case, dtype, r, stored, din, rows.double().sum(1))


@pytest.mark.parametrize("with_affine", [True, False], ids=["affine", "plain"])
@pytest.mark.parametrize("c,cp", R.FIN_CHANNELS)
@pytest.mark.parametrize("tiles", R.FIN_TILES)
def test_finalize_emulation_passes(tiles, c, cp, with_affine):
    part = R.finalize_partials(tiles, c, cp)
    gamma, beta = R.finalize_affine(c) if with_affine else (None, None)
    vox = R.FIN_TILE_VOX * tiles
    assert np.isnan(part[:, :, c:]).all() and np.isfinite(part[:, :, :c]).all()
    R.check_finalize("in_finalize", emu_finalize(part, c, cp, vox, gamma, beta), part, c, vox, gamma, beta)


def test_the_second_constant_channel_has_a_negative_variance_before_the_clamp():
    n, ch, _ = R.NEG_VAR_CHANNEL
    for tiles in R.FIN_TILES:
        s = R.finalize_partials(tiles, 32, 32)[n, :, ch].astype(np.float64).sum(0)
        vox = R.FIN_TILE_VOX * tiles
        assert s[1] / vox - (s[0] / vox) ** 2 < -1e-9


# ------------------------------------------------------------------------------------------------ the defects fail
def _enc(case, dtype):
    n, c, ho, wo, bias = R.ENC_TAIL[case]
    return R.enc_tail_case(dtype, n, c, ho, wo), bias


def _ups(case, dtype):
    n, c, hi, wi, bias = R.UPSAMPLE[case]
    return R.upsample_case(dtype, n, c, hi, wi), bias


def _pool(case, dtype):
    n, c, ho, wo, _ = R.POOL_BWD[case]
    r = R.pool_bwd_case(dtype, n, c, ho, wo)
    stored, _, idx = emu_enc_tail(r, dtype)
    return r, stored, idx


@pytest.mark.parametrize("dtype", HALF, ids=IDS)
def test_truncating_stores_are_rejected(dtype):
    """by the elementwise bound AND, alone, by the bias statistic"""
    r, _ = _enc("base", dtype)
    ds, pooled, idx = emu_enc_tail(r, dtype, trunc=True)
    u, _ = _ups("base", dtype)
    p, stored, pidx = _pool("row1", dtype)
    din, _ = emu_pool_bwd(p, pidx, dtype, trunc=True)
    for got, ref64, acc in ((ds, r["ref64"], r["acc"]), (emu_upsample(u, dtype, trunc=True), u["ref64"], u["acc"]),
                            (emu_adjoint(u, dtype, trunc=True), u["adj64"], u["adj_acc"]),
                            (din, *R.pool_bwd_reference(p, stored))):
        with pytest.raises(AssertionError, match="outside the bound"):
            R.check_rounded(got, ref64, dtype, acc)
        with pytest.raises(AssertionError, match="signed rounding bias"):
            R.check_rounding_bias(got, ref64, dtype)


@pytest.mark.parametrize("dtype", R.ALL, ids=IDS)
@pytest.mark.parametrize("case", ["h1", "w1"])
def test_zero_padded_bilinear_edges_are_rejected(case, dtype):
    r, bias = _ups(case, dtype)
    with pytest.raises(AssertionError, match="outside the bound"):
        R.held("zero_pad", dtype, emu_upsample(r, dtype, zero_pad=True), r["ref64"], r["acc"], bias)


@pytest.mark.parametrize("dtype", R.ALL, ids=IDS)
def test_swapped_bilinear_weights_are_rejected(dtype):
    r, bias = _ups("h1", dtype)
    with pytest.raises(AssertionError, match="outside the bound"):
        R.held("swap", dtype, emu_upsample(r, dtype, swap=True), r["ref64"], r["acc"], bias)


@pytest.mark.parametrize("dtype", R.ALL, ids=IDS)
def test_an_adjoint_without_one_border_row_of_taps_is_rejected(dtype):
    r, bias = _ups("h1", dtype)
    with pytest.raises(AssertionError, match="outside the bound"):
        R.held("border", dtype, emu_adjoint(r, dtype, drop_border=True), r["adj64"], r["adj_acc"], bias)


@pytest.mark.parametrize("dtype", R.ALL, ids=IDS)
def test_wrong_window_indices_are_rejected(dtype):
    r, bias = _enc("one_window", dtype)
    with pytest.raises(AssertionError, match="window indices differ"):
        R.check_enc_tail("transposed", dtype, r, *emu_enc_tail(r, dtype, transposed_index=True), bias)
    with pytest.raises(AssertionError, match="window indices differ"):
        R.check_enc_tail("last", dtype, r, *emu_enc_tail(r, dtype, keep_last=True), bias)
    ds, pooled, idx = emu_enc_tail(r, dtype)
    with pytest.raises(AssertionError, match="index above 3"):
        R.check_enc_tail("byte", dtype, r, ds, pooled, idx + 4 * (idx == 1).to(torch.uint8), bias)
    with pytest.raises(AssertionError, match="not the maximum"):
        R.check_enc_tail("pooled", dtype, r, ds, ds[:, :, ::2, ::2].contiguous(), idx, bias)


@pytest.mark.parametrize("dtype", R.ALL, ids=IDS)
def test_a_scatter_that_drops_the_old_gradient_is_rejected(dtype):
    r, stored, idx = _pool("row1", dtype)
    din, rows = emu_pool_bwd(r, idx, dtype, without_old=True)
    with pytest.raises(AssertionError, match="outside the bound"):
        R.check_pool_bwd("without_old", dtype, r, stored, din, rows.double().sum(1))


@pytest.mark.parametrize("dtype", R.ALL, ids=IDS)
def test_an_unsummed_or_unwritten_partial_row_is_rejected(dtype):
    r, stored, idx = _pool("lanes21", dtype)
    din, rows = emu_pool_bwd(r, idx, dtype, skip_last_row=True)
    with pytest.raises(AssertionError, match="row sums"):
        R.check_pool_bwd("last_row", dtype, r, stored, din, rows.double().sum(1))
    din, rows = emu_pool_bwd(r, idx, dtype)
    rows[1, 0] = float("nan")
    with pytest.raises(AssertionError, match="was not written"):
        R.check_pool_bwd("nan_row", dtype, r, stored, din, rows.double().sum(1))


@pytest.mark.parametrize("defect,tiles,ccp", [(dict(unbiased=True), 1, (32, 32)), (dict(clamp=False), 1, (32, 32)),
                                              (dict(remainder=False), 129, (32, 32)), (dict(pitch=48), 31, (48, 64))],
                         ids=["unbiased", "no_clamp", "no_remainder", "pitch_c"])
def test_finalize_defects_are_rejected(defect, tiles, ccp):
    c, cp = ccp
    part = R.finalize_partials(tiles, c, cp)
    gamma, beta = R.finalize_affine(c)
    vox = R.FIN_TILE_VOX * tiles
    got = emu_finalize(part, c, cp, vox, gamma, beta, **defect)
    with pytest.raises(AssertionError, match="x its bound"):
        R.check_finalize("defect", got, part, c, vox, gamma, beta)
    if "clamp" in defect:      # only the channel with the negative variance shows it
        n, ch, _ = R.NEG_VAR_CHANNEL
        ref, bound = R.finalize_bounds(part, c, vox, gamma, beta, R.EPS)["rstd"]
        bad = ~(np.abs(got["rstd"].astype(np.float64) - ref) <= bound)
        assert bad[n, ch] and bad.sum() == 1
