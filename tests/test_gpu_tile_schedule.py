"""The tile schedule of the persistent conv kernels (csrc/conv_schedule.h; conv_ws2_kernel carries its own copy of it, held
to the same results here) on the device, on the paths no other test reaches:
an interior pass (three or more tiles per axis: 48^3 is a 12x6x6 grid of 4x8x8 tiles, 47x50x49 a ragged 12x7x7 one), two
samples so both tile lists cross a sample, and compute-unit budgets (hdf_set_cu_budget) that change gridDim.x -- among them
grids that are no multiple of 8, which the kernels walk as ONE range instead of one per XCD.

gridDim.x per budget (864 tiles at 48^3, 1176 at 47x50x49):
  conv_ws2_kernel 32 -> 32   one output-channel tile: gridDim.x = budget, and a budget is a multiple of 8 -- 256, 24, 40 walk
                             8 ranges with 32, 3 and 5 workgroups each; the single range is reached by the next case
  conv_ws2_kernel 64 -> 128  four channel tiles: 64, 6, 10
  conv_wr_kernel 64 -> 64    two channel tiles: 128, 12, 20
  conv_wgrad2_kernel 32 x 32 gridDim.x = ceil(tiles / ceil(tiles / budget)): 216, 24, 79 at 48^3 and 236, 24, 79 ragged
Each result meets the tolerance tests/test_gpu_ops.py holds the entry to, against torch's fp32 conv on the storage-rounded
operands; the output is prefilled with NaN so a tile nobody visits shows; the forward outputs are equal bit for bit under the
three budgets (the budget changes which workgroup computes a tile, never the order inside it; the weight gradient is summed
across workgroups and is held to the tolerance only)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from hdf_rt._lib import BF16, check, lib, ptr  # noqa: E402
from hip_util import DEV, conv3d, from_cl, pack_w, rel_err, rnd, rup, st, to_cl  # noqa: E402

TOL = 2e-2          # bf16 storage: tests/test_gpu_ops.py TOL[BF16]
EXTENTS = [(48, 48, 48), (47, 50, 49)]
N = 2


def _mk(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g)


def _under_budgets(budgets, run):
    outs = []
    try:
        for b in budgets:
            check(lib().hdf_set_cu_budget(b), "budget")
            outs.append(run())
            torch.cuda.synchronize()
    finally:
        check(lib().hdf_set_cu_budget(256), "budget")
    return outs


def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("size", EXTENTS)
@pytest.mark.parametrize("kernel,cin,cout,budgets", [("ws2", 32, 32, (256, 24, 40)), ("ws2", 64, 128, (256, 24, 40)),
                                                     ("wr", 64, 64, (256, 24, 40))])
def test_forward_kernels_under_cu_budgets(kernel, cin, cout, budgets, size):
    dtype = BF16
    x, w, b = _mk((N, cin) + size, 31), _mk((cout, cin, 3, 3, 3), 32) * (cin * 27) ** -0.5, _mk((cout,), 33)
    ref = F.conv3d(rnd(x, dtype).to(DEV), rnd(w, dtype).to(DEV), b.to(DEV), padding=1).cpu()
    wp = pack_w(w, dtype, cout, cin, rup(cout, 32), cin, cin * 27, 27, 0)
    x_cl, bias = to_cl(x, dtype), b.to(DEV)

    def run():
        out = torch.full((N,) + size + (cout,), float("nan"), dtype=x_cl.dtype, device=DEV)
        if kernel == "wr":
            check(lib().hdf_op_conv3d_wr(dtype, ptr(x_cl), cin, cin, N, *size, ptr(wp), ptr(bias), None, None, 0, ptr(out),
                                         cout, cout, None, 0, st()), "conv3d_wr")
        else:
            conv3d(dtype, 0, x_cl, cin, wp, cout, bias=bias, out=out, out_pitch=cout)
        return out

    outs = _under_budgets(budgets, run)
    for bud, out in zip(budgets, outs):
        got = from_cl(out)
        assert rel_err(got, ref) < TOL, bud          # (a NaN left by an unvisited tile compares false)
    for bud, out in zip(budgets[1:], outs[1:]):
        assert torch.equal(_bits(out), _bits(outs[0])), "budget %d: output differs from budget %d's" % (bud, budgets[0])


@pytest.mark.parametrize("size", EXTENTS)
def test_weight_gradient_under_cu_budgets(size):
    dtype, cin, cout, budgets = BF16, 32, 32, (256, 24, 80)
    x, dy = _mk((N, cin) + size, 41), _mk((N, cout) + size, 42)
    w = torch.zeros(cout, cin, 3, 3, 3, requires_grad=True, device=DEV)
    F.conv3d(rnd(x, dtype).to(DEV), w, None, padding=1).backward(rnd(dy, dtype).to(DEV))
    ref = w.grad.cpu()
    s_cl, l_cl = to_cl(dy, dtype), to_cl(x, dtype)
    wsb = lib().hdf_op_wgrad_workspace_bytes(1, N, *size, cout, cin)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)

    def run():
        dw = torch.full((cout, cin, 27), float("nan"), dtype=torch.float32, device=DEV)
        check(lib().hdf_op_conv3d_wgrad(dtype, 1, ptr(s_cl), cout, cout, ptr(l_cl), cin, cin, N, *size, None, None, 0, None,
                                        None, 0, ptr(dw), cout, cin, 0, ptr(ws), wsb, st()), "wgrad")
        return dw

    for bud, dw in zip(budgets, _under_budgets(budgets, run)):
        assert rel_err(dw.cpu().view(cout, cin, 3, 3, 3), ref) < TOL, bud
