"""Self-tests of the rounding-aware comparison of tests/hip_util.py (check_rounded, check_fp32_sum, check_rounding_bias),
on the CPU alone: the reference's own output, rounded to nearest-even, is accepted; three planted defects are rejected --
a store that truncates instead of rounding, one corner voxel of dy left out of a weight gradient, one 3x3x3 tap skipped on
one boundary plane of a forward conv -- and the first two pass the metric the operator tests used alone before
(rel_err = max error / max reference at 2e-2 for bf16, 3e-3 for float16), which is why the sharper gate exists.
Shapes: those of test_gpu_ops.py test_conv3d_s1 / test_conv3d_wgrad.  acc = 4 * max|fp32 op - fp64 op| as in the GPU module."""
import pytest
import torch
import torch.nn.functional as F

from hdf_rt._lib import BF16, F16, F32
from hip_util import (TDT, check_fp32_sum, check_rounded, check_rounding_bias, rel_err, rnd, rounding_excess,
                      signed_rounding_bias, ulp_of)

OLD_TOL = {BF16: 2e-2, F16: 3e-3}
SHAPES = [(32, 32, (12, 16, 24), 2), (128, 96, (6, 10, 9), 2)]


def _mk(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _truncate(r32, dtype):
    """fp32 -> storage type by dropping the low bits (round toward zero), returned as fp32"""
    mask = ~0xFFFF if dtype == BF16 else ~0x1FFF
    return (r32.contiguous().view(torch.int32) & mask).view(torch.float32)


def _conv(dtype, cin, cout, size, n):
    x = rnd(_mk((n, cin) + size, 1), dtype)
    w = rnd(_mk((cout, cin, 3, 3, 3), 2) * (cin * 27) ** -0.5, dtype)
    b = _mk((cout,), 3)
    r64 = F.conv3d(x.double(), w.double(), b.double(), padding=1)
    r32 = F.conv3d(x, w, b, padding=1)
    return x, w, r32, r64, 4 * float((r32.double() - r64).abs().max())


def test_ulp_of_matches_the_storage_types():
    for dtype in (BF16, F16):
        v = torch.tensor([1.0, 1.5, 2.0, 0.75, -3.0, 100.0, 2.0 ** -14, 2.0 ** -10], dtype=torch.float64)
        nxt = torch.nextafter(v.abs().to(TDT[dtype]), torch.tensor(float("inf"), dtype=TDT[dtype])).double()
        assert torch.equal(ulp_of(v, dtype), nxt - v.abs())
    assert float(ulp_of(torch.tensor([0.0, 1e-9, 2.0 ** -15], dtype=torch.float64), F16).max()) == 2.0 ** -24
    assert float(ulp_of(torch.tensor([1.0], dtype=torch.float64), F32)) == 2.0 ** -23
    assert float(ulp_of(torch.tensor([1.0], dtype=torch.float64), BF16)) == 2.0 ** -7
    assert float(ulp_of(torch.tensor([1.99], dtype=torch.float64), F16)) == 2.0 ** -10


@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("cin,cout,size,n", SHAPES)
def test_round_to_nearest_is_accepted_and_a_truncating_store_is_rejected(dtype, cin, cout, size, n):
    _, _, r32, r64, acc = _conv(dtype, cin, cout, size, n)
    rne = rnd(r32, dtype)
    assert check_rounded(rne, r64, dtype, acc) <= 1.0
    check_rounding_bias(rne, r64, dtype)
    trunc = _truncate(r32, dtype)
    assert rel_err(trunc, r32) < OLD_TOL[dtype]                      # the old gate lets it through ...
    with pytest.raises(AssertionError, match="outside the bound"):  # ... the elementwise bound does not
        check_rounded(trunc, r64, dtype, acc)
    assert float((rounding_excess(trunc, r64, dtype, acc) > 1).double().mean()) > 0.3
    bias, used, total = signed_rounding_bias(trunc, r64, dtype)
    assert bias < -0.45 and used >= 0.9 * total
    with pytest.raises(AssertionError, match="signed rounding bias"):
        check_rounding_bias(trunc, r64, dtype)


@pytest.mark.parametrize("dtype", [BF16, F16])
def test_a_tap_skipped_on_one_boundary_plane_is_rejected(dtype):
    cin, cout, size, n = SHAPES[0]
    x, w, r32, r64, acc = _conv(dtype, cin, cout, size, n)
    one = torch.zeros_like(w)
    one[:, :, 0, 0, 0] = w[:, :, 0, 0, 0]
    bad = r32.clone()
    bad[:, :, -1] -= F.conv3d(x, one, None, padding=1)[:, :, -1]    # the last z plane never reads tap (0, 0, 0)
    with pytest.raises(AssertionError) as err:
        check_rounded(rnd(bad, dtype), r64, dtype, acc)
    assert "worst at index" in str(err.value)
    ratio = rounding_excess(rnd(bad, dtype), r64, dtype, acc)
    assert bool((ratio[:, :, :-1] <= 1).all()) and float((ratio[:, :, -1] > 1).double().mean()) > 0.5   # the plane shows


@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("cin,cout,size,n", SHAPES)
def test_a_corner_voxel_dropped_from_a_weight_gradient_is_rejected(dtype, cin, cout, size, n):
    x, dy = rnd(_mk((n, cin) + size, 13), dtype), rnd(_mk((n, cout) + size, 14), dtype)

    def wgrad(xx, dd):
        wz = torch.zeros(cout, cin, 3, 3, 3, dtype=xx.dtype, requires_grad=True)
        F.conv3d(xx, wz, None, padding=1).backward(dd)
        return wz.grad

    g64, g32 = wgrad(x.double(), dy.double()), wgrad(x, dy)
    acc = 4 * float((g32.double() - g64).abs().max())
    assert check_fp32_sum(g32, g64, acc) <= 1.0
    dropped = dy.clone()
    dropped[0, :, -1, -1, -1] = 0
    bad = wgrad(x, dropped)
    if dtype == BF16 and size == SHAPES[0][2]:
        assert rel_err(bad, g32) < OLD_TOL[dtype]                    # under the old gate: 1.5e-2 against 2e-2
    with pytest.raises(AssertionError, match="outside the bound"):
        check_fp32_sum(bad, g64, acc)


def test_a_nan_output_is_rejected():
    r64 = torch.ones(4, dtype=torch.float64)
    got = torch.ones(4)
    got[2] = float("nan")
    with pytest.raises(AssertionError):
        check_rounded(got, r64, BF16, 0.0)
    with pytest.raises(AssertionError):
        check_fp32_sum(got, r64, 0.0)
