"""The 2-D (FLAT) pooling / up-sampling kernels of csrc/pool_ops.hip and the InstanceNorm statistics' finalize
(csrc/norm_ops.hip in_finalize_kernel) held to fp64 at the operator level, as test_gpu_ops_rounding.py holds their 3-D
siblings.  The 2-D plan runs all four FLAT forms in every step; before this file only the whole-model comparisons of
test_gpu_model_2d.py saw them (1e-3 .. 3e-2 rel-L2, which a truncating store or a dropped edge row passes).

The reference side, the data of the cases and the checks are tests/pool2d_ref.py; tests/test_pool2d_ref_cpu.py shows on the
CPU that the checks reject a truncating store of ds / the up-sampled tensor / the adjoint / din, zero-padded or swapped
bilinear edges, the window index as 2 dx + dy, the last maximum on ties, a border row of adjoint taps left out, a scatter
without the old din, an unsummed partial row, and a finalize with the unbiased variance / no clamp / no remainder loop /
pitch C.

Bounds: hip_util.check_rounded, |got - ref64| <= 0.5 ulp of the storage type + acc with
acc = 4 x max|op in torch fp32 - op in torch fp64| on the same storage-rounded operands (nothing from the kernel), and
check_rounding_bias on every 16-bit tensor of 10 000 elements and more.  pooled and idx are compared EXACTLY with
F.max_pool2d(return_indices) of the returned ds (the kernel pools the stored values).  The partial rows of
hdf_op_maxpool_bwd_in_2d, summed in fp64 over the rows of a sample, are held per (n, c) to 4 x the fp32-vs-fp64 spread of the
same sums of the returned din on the CPU, plus |g| resp. |g xhat| of the elements whose mask y * scale + shift > 0 differs
between fp64 (an fma) and unfused fp32 (fewer than 1 in 1000: a condition on the data, asserted).  The finalize's bounds
are in pool2d_ref's docstring.  Every output has a guard tail of 64 elements of 7.0, and in one case per entry every
operand is the upper half of a 2C row whose lower half is 7.0; both are checked untouched.  No case needed a factor above
4, no element is excluded.

route -> case (bf16, f16 and f32 throughout):
  enc_tail_kernel<T, true>            test_encoder_tail_2d[base]       (2, 32, 12 x 20 pooled) 61,440 elements of ds
                                      [c48_odd]    (2, 48, 9 x 13)   C / EPC no power of two, odd pooled extents, 2C pitch
                                      [one_window] (3, 16, 1 x 1)    one window per sample (no bias statistic: 192 elements)
                                      channel 0 of every case: ds = 0 throughout, every window a tie, idx = 0
  upsample_fwd_kernel<T, true> and    test_upsample_2d[base]           (2, 32, 24 x 40)
  upsample_bwd_kernel<T, true>        [odd]        (3, 16, 17 x 23)  odd extents, 51 workgroups: identity slab order, 2C pitch
                                      [gx2_slab]   (2, 64, 12 x 40)  bf16 / f16: 320 chunks per row, gx = 2, 48 workgroups:
                                                                     permuted slab order
                                      [h1], [w1]   (2, 16, 1 x 9), (2, 16, 9 x 1)  both clamped neighbours on one axis (no
                                                                     bias statistic: 1,152 elements)
  maxpool_bwd_inb_kernel<T, true>     test_maxpool_backward_in_2d[rows4]   (2, 32, 25 x 41)  4 rows of 257 / 257 / 257 / 254
                                      [lanes21]    (2, 48, 19 x 25)  21 voxel lanes, threads 252..255 idle, rows of 238 / 237,
                                                                     2C pitch
                                      [row1]       (3, 16, 6 x 10)   64 lanes, one row
                                      idx and the stored ds come from hdf_op_enc_tail_2d on the same data
  in_finalize_kernel                  test_in_finalize[tiles x (C, CP) x affine]: tiles 1, 31 (fewer than one lane pass),
                                      33 (remainder loop only), 128 (one unrolled group), 129, 515 (groups + remainder);
                                      (C, CP) = (32, 32), (48, 64), (63, 64) with NaN in channels C..CP-1; gamma / beta given
                                      and null; a constant channel (var = 0, rstd = 1 / sqrt(eps)) and one whose fp32 sum
                                      of squares lies below vox * value^2 (var < 0 before the clamp)
Each check prints one line "ROUNDING <case> <worst error / bound>" (pytest -s shows them).

MEASURED on an MI355X, worst error / bound per check, factor 4 everywhere.  A 16-bit store shows a ratio near 1 because
half an ulp of the storage type is most of its bound; the fp32 column shows what the arithmetic uses of acc.  The torch
emulation of the kernels' order of operations on the CPU (test_pool2d_ref_cpu.py) gives row figures of the same size
(0.09 .. 0.63) and the same finalize figures.
                                       f32     bf16    f16
  enc_tail_2d.base.ds                  0.191   1.000   0.998
  enc_tail_2d.c48_odd.ds               0.211   1.000   0.999
  enc_tail_2d.one_window.ds            0.207   0.993   0.998
  upsample_fwd_2d.base                 0.219   1.000   0.999
  upsample_fwd_2d.odd                  0.285   1.000   0.998
  upsample_fwd_2d.gx2_slab             0.233   1.000   0.998
  upsample_fwd_2d.h1 / .w1             0.294   0.999   0.997
  upsample_bwd_2d.base                 0.235   1.000   0.999
  upsample_bwd_2d.odd                  0.236   1.000   0.999
  upsample_bwd_2d.gx2_slab             0.235   1.000   0.999
  upsample_bwd_2d.h1 / .w1             0.135   1.000   1.000
  maxpool_bwd_in_2d.*.din              0.200   1.000   1.000    (d0 + g is exact in fp32: rounding ties sit on the bound)
  maxpool_bwd_in_2d.rows4.row0 / row1  0.355 / 0.478   0.125 / 0.329   0.153 / 0.634
  maxpool_bwd_in_2d.lanes21.row0 / 1   0.549 / 0.299   0.094 / 0.216   0.139 / 0.307
  maxpool_bwd_in_2d.row1.row0 / row1   0.450 / 0.539   0.000 / 0.480   0.000 / 0.501    (240 16-bit terms sum exactly)
  in_finalize (36 cases)               mean 1.000   rstd 1.000   scale 0.938   shift 0.423    (mean and rstd are one fp32
                                       rounding of the fp64 value: exactly half an ulp at worst, by construction)
pooled, idx, the guard tails, the neighbouring channel slices and the inputs compared exactly in every case.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import pool2d_ref as R  # noqa: E402
from hdf_rt._lib import check, lib, ptr  # noqa: E402
from hip_util import DEV, TDT, st  # noqa: E402

IDS = R.NAME.get
G = R.GUARD


class Buf:
    """channels-last storage [N][H][W][pitch] with a guard tail, everything 7.0 until written.  wide: the tensor is the
    upper half of a 2C row (pitch 2C); the lower half and the tail must stay 7.0"""

    def __init__(self, n, h, w, c, tdt, wide=False, value=None):
        self.c, self.pitch, self.lead = c, (2 * c if wide else c), (c if wide else 0)
        self.numel = n * h * w * self.pitch
        self.flat = torch.full((self.numel + G,), 7.0, dtype=tdt, device=DEV)
        self.full = self.flat[:self.numel].view(n, h, w, self.pitch)
        self.view = self.full[..., self.lead:]
        if value is not None:       # [N, C, H, W] on the CPU
            self.view.copy_(value.permute(0, 2, 3, 1).to(tdt).to(DEV))

    def ptr(self):
        return self.flat[self.lead:].data_ptr()

    def get(self):
        """[N, C, H, W] on the CPU, after checking what surrounds the tensor"""
        assert bool((self.flat[self.numel:] == 7.0).all()), "the guard tail was written"
        assert bool((self.full[..., :self.lead] == 7.0).all()), "the neighbouring channel slice was written"
        v = self.view.permute(0, 3, 1, 2).contiguous().cpu()
        return v if v.dtype == torch.uint8 else v.float()


def _dev(*ts):
    return [t.to(DEV).contiguous() for t in ts]


def _run_enc_tail(dtype, r, wide):
    n, c, h, w = r["y"].shape
    tdt = TDT[dtype]
    y, skip = Buf(n, h, w, c, tdt, wide, r["y"]), Buf(n, h, w, c, tdt, wide, r["skip"])
    ds, pooled = Buf(n, h, w, c, tdt, wide), Buf(n, h // 2, w // 2, c, tdt, wide)
    idx = Buf(n, h // 2, w // 2, c, torch.uint8)            # (idx has no pitch: [N][Ho][Wo][C] bytes)
    sc, sh = _dev(r["scale"], r["shift"])
    check(lib().hdf_op_enc_tail_2d(dtype, y.ptr(), y.pitch, ptr(sc), ptr(sh), skip.ptr(), skip.pitch, ds.ptr(), ds.pitch,
                                   pooled.ptr(), pooled.pitch, idx.ptr(), n, c, h // 2, w // 2, st()), "enc_tail_2d")
    torch.cuda.synchronize()
    assert torch.equal(y.get(), r["y"]) and torch.equal(skip.get(), r["skip"])      # the inputs are only read
    return ds.get(), pooled.get(), idx.get()


@pytest.mark.parametrize("dtype", R.ALL, ids=IDS)
@pytest.mark.parametrize("case", list(R.ENC_TAIL))
def test_encoder_tail_2d(case, dtype):
    n, c, ho, wo, bias = R.ENC_TAIL[case]
    r = R.enc_tail_case(dtype, n, c, ho, wo)
    ds, pooled, idx = _run_enc_tail(dtype, r, R.PITCHED["enc_tail"] == case)
    R.check_enc_tail("enc_tail_2d." + case, dtype, r, ds, pooled, idx, bias)


@pytest.mark.parametrize("dtype", R.ALL, ids=IDS)
@pytest.mark.parametrize("case", list(R.UPSAMPLE))
def test_upsample_2d(case, dtype):
    """hdf_op_upsample_fwd_2d: bilinear x2 of relu(x * scale + shift); hdf_op_upsample_bwd_2d: its adjoint, the gradient read
    from the upper half of a 2C row"""
    n, c, hi, wi, bias = R.UPSAMPLE[case]
    wide = R.PITCHED["upsample"] == case
    r = R.upsample_case(dtype, n, c, hi, wi)
    tdt = TDT[dtype]
    x, up = Buf(n, hi, wi, c, tdt, wide, r["x"]), Buf(n, 2 * hi, 2 * wi, c, tdt, wide)
    sc, sh = _dev(r["scale"], r["shift"])
    check(lib().hdf_op_upsample_fwd_2d(dtype, x.ptr(), x.pitch, ptr(sc), ptr(sh), up.ptr(), up.pitch, n, c, hi, wi, st()),
          "upsample_fwd_2d")
    g, din = Buf(n, 2 * hi, 2 * wi, c, tdt, True, r["g"]), Buf(n, hi, wi, c, tdt, wide)
    check(lib().hdf_op_upsample_bwd_2d(dtype, g.ptr(), g.pitch, din.ptr(), din.pitch, n, c, hi, wi, st()),
          "upsample_bwd_2d")
    torch.cuda.synchronize()
    assert torch.equal(x.get(), r["x"]) and torch.equal(g.get(), r["g"])
    R.held("upsample_fwd_2d." + case, dtype, up.get(), r["ref64"], r["acc"], bias)
    R.held("upsample_bwd_2d." + case, dtype, din.get(), r["adj64"], r["adj_acc"], bias)


@pytest.mark.parametrize("dtype", R.ALL, ids=IDS)
@pytest.mark.parametrize("case", list(R.POOL_BWD))
def test_maxpool_backward_in_2d(case, dtype):
    """hdf_op_maxpool_bwd_in_2d: din = RNE(float(din) + scatter(dout)) at the maxima hdf_op_enc_tail_2d found, and the rows
    (sum g, sum g * xhat) of the stored din, every row written"""
    n, c, ho, wo, nrows = R.POOL_BWD[case]
    wide = R.PITCHED["pool_bwd"] == case
    assert lib().hdf_op_maxpool_bwd_in_rows(c, 1, ho, wo) == nrows == R.rows_per_sample(c, ho * wo)
    r = R.pool_bwd_case(dtype, n, c, ho, wo)
    stored, _, idx_cpu = _run_enc_tail(dtype, r, False)
    assert int(idx_cpu[:, 0].max()) == 0                    # the all-tie channel
    tdt = TDT[dtype]
    h, w = 2 * ho, 2 * wo
    idx = idx_cpu.permute(0, 2, 3, 1).contiguous().to(DEV)
    g, din, y = Buf(n, ho, wo, c, tdt, wide, r["g"]), Buf(n, h, w, c, tdt, wide, r["d0"]), Buf(n, h, w, c, tdt, wide, r["y"])
    part = torch.full((n * nrows * c * 2 + G,), float("nan"), device=DEV)
    part[-G:] = 7.0
    vec = _dev(r["scale"], r["shift"], r["mean"], r["rstd"])
    check(lib().hdf_op_maxpool_bwd_in_2d(dtype, g.ptr(), g.pitch, ptr(idx), din.ptr(), din.pitch, y.ptr(), y.pitch,
                                         *[ptr(v) for v in vec], ptr(part), n, c, ho, wo, st()), "maxpool_bwd_in_2d")
    torch.cuda.synchronize()
    assert torch.equal(g.get(), r["g"]) and torch.equal(y.get(), r["y"])
    assert bool((part[-G:] == 7.0).all()), "the guard tail of the partial rows was written"
    rows = part[:-G].view(n, nrows, c, 2).cpu()
    assert bool(torch.isfinite(rows).all()), "a partial row was not written"
    got = din.get()
    flipped = R.first_pass(got, r["y"], r["scale"], r["shift"], r["mean"], r["rstd"])[2]
    assert flipped < 1e-3, flipped
    R.check_pool_bwd("maxpool_bwd_in_2d." + case, dtype, r, stored, got, rows.double().sum(1))


@pytest.mark.parametrize("with_affine", [True, False], ids=["affine", "plain"])
@pytest.mark.parametrize("c,cp", R.FIN_CHANNELS)
@pytest.mark.parametrize("tiles", R.FIN_TILES)
def test_in_finalize(tiles, c, cp, with_affine):
    """hdf_op_in_finalize: mean / rstd / scale / shift [N][C] from fp32 partial rows [N][tiles][CP][2]"""
    part = R.finalize_partials(tiles, c, cp)
    gamma, beta = R.finalize_affine(c) if with_affine else (None, None)
    n, vox = R.FIN_N, R.FIN_TILE_VOX * tiles
    pd = torch.from_numpy(part).to(DEV).contiguous()
    gd, bd = (torch.from_numpy(gamma).to(DEV), torch.from_numpy(beta).to(DEV)) if with_affine else (None, None)
    out = {k: torch.full((n * c + G,), 7.0, device=DEV) for k in ("mean", "rstd", "scale", "shift")}
    check(lib().hdf_op_in_finalize(ptr(pd), n, tiles, c, cp, vox, ptr(gd), ptr(bd), R.EPS, ptr(out["mean"]),
                                   ptr(out["rstd"]), ptr(out["scale"]), ptr(out["shift"]), st()), "in_finalize")
    torch.cuda.synchronize()
    assert np.array_equal(pd.cpu().numpy(), part, equal_nan=True)
    got = {}
    for k, v in out.items():
        assert bool((v[n * c:] == 7.0).all()), "the guard tail of %s was written" % k
        got[k] = v[:n * c].view(n, c).cpu().numpy()
    R.check_finalize("in_finalize.t%d.c%d_%d.%s" % (tiles, c, cp, "affine" if with_affine else "plain"), got, part, c, vox,
                     gamma, beta)
