"""TopKLoss on the device (hdf_loss_topk_*, hdf_op_topk_select; reference loss/cross_entropy.py:26-43): the select exact
in every bit against numpy, the loss and its gradient for every case x dtype x form against the restatement of
tests/topk_ref.py (allowances, guard band and checking functions: tests/test_topk_ref_cpu.py proves them on planted
defects), the reference's own recorded vectors (g12_topk_loss), and one step through the model."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from conftest import GOLDEN  # noqa: E402

import topk_ref as tr  # noqa: E402
from hdf_rt._lib import BF16, F16, F32, check, lib, ptr  # noqa: E402
from hip_util import TDT, check_rounded, st  # noqa: E402

DEV = "cuda:0"
PAIRS = [(c, d) for c in tr.CASES for d in tr.DTYPES]
IDS = ["%s-%s" % (c, tr.NAME[d]) for c, d in PAIRS]
SELECT_WS = 65536


# ================================================================================================ the select
def run_select(values, K, want=("rank", "values", "mean")):
    """hdf_op_topk_select on a device tensor -> (result[4], rank, values_out, mean) on the host"""
    n = values.numel()
    ws = torch.empty(SELECT_WS, dtype=torch.uint8, device=DEV)
    result = torch.full((4,), -1, dtype=torch.int64, device=DEV)
    rank = torch.full((n,), -7, dtype=torch.int32, device=DEV) if "rank" in want else None
    vout = torch.full((K,), -7.0, dtype=torch.float32, device=DEV) if "values" in want else None
    mean = torch.full((1,), -7.0, dtype=torch.float32, device=DEV) if "mean" in want else None
    check(lib().hdf_op_topk_select(ptr(values), n, K, ptr(ws), ws.numel(), ptr(result), ptr(rank), ptr(vout), ptr(mean), st()),
          "hdf_op_topk_select")
    torch.cuda.synchronize()
    host = lambda t: None if t is None else t.cpu().numpy()
    return host(result), host(rank), host(vout), host(mean)


def select_twice_and_check(v, K):
    dv = torch.from_numpy(v).to(DEV)
    a = run_select(dv, K)
    b = run_select(dv, K)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes(), "two runs differ"
    tr.check_select_exact(v, K, a[0], a[1], a[2], a[3][0])
    return a


@functools.lru_cache(maxsize=None)
def normal_values(n):
    return torch.randn(n, generator=torch.Generator().manual_seed(90 + n % 97)).numpy()


SIZES = [1, 255, 256, 257, 5000011]          # the last is beyond any grid cap: every grid-stride loop runs more than once


@pytest.mark.parametrize("n", SIZES)
def test_select_is_exact_at_every_size_and_k(n):
    v = normal_values(n)
    for K in sorted({1, n - 1, n, n // 10} - {0}):
        res, *_ = select_twice_and_check(v, K)
        print("  n %d K %d: threshold bits %#x above %d ties %d" % (n, K, res[0], res[1], res[2]))


def test_select_with_thousands_of_ties_at_the_threshold():
    v = (torch.randint(0, 7, (100003,), generator=torch.Generator().manual_seed(5)).float() * 0.25 - 0.5).numpy()
    for K in (1, 10000, 50000, 100003):
        res, *_ = select_twice_and_check(v, K)
        assert K in (1, 100003) or res[2] > 1000


def test_select_all_values_equal():
    v = np.full(70001, 1.5, dtype=np.float32)
    res, rank, vout, mean = select_twice_and_check(v, 12345)
    assert list(res) == [0x3FC00000, 0, 12345, 0] and int(rank[12344]) == 12344 and int(rank[12345]) == -1
    select_twice_and_check(np.zeros(300, dtype=np.float32), 300)
    select_twice_and_check(-np.zeros(300, dtype=np.float32), 7)


def test_select_each_radix_pass_decides_alone():
    g = torch.Generator().manual_seed(11)
    low = (torch.randint(0, 1024, (30011,), generator=g).int() | 0x3F800000).numpy().view(np.float32)      # lowest 10 bits
    mid = ((torch.randint(0, 2048, (30011,), generator=g).int() << 10) | 0x3F800000).numpy().view(np.float32)
    r = torch.randint(0, 2048, (30011,), generator=g).int()
    r = torch.where((r & 1023) >= 1020, r - 8, r)                                                           # no inf / NaN
    top = (r.long() << 21).numpy().astype(np.uint32).view(np.float32)                                       # top 11 bits
    for v in (low, mid, top):
        for K in (1, 3001, 30011):
            select_twice_and_check(v, K)


def test_select_inf_and_nan_nan_comes_first():
    v = normal_values(4099).copy()
    v[17], v[4000] = np.inf, -np.inf
    u = v.view(np.uint32)
    u[100], u[3000] = 0x7FC00001, 0xFFC00000          # a positive NaN with a payload and a negative one
    res, rank, vout, mean = select_twice_and_check(v, 2)
    assert list(res[:3]) == [0x7FC00000, 0, 2] and int(rank[100]) == 0 and int(rank[3000]) == 1 and np.isnan(mean[0])
    assert vout.view(np.uint32).tolist() == [0x7FC00001, 0xFFC00000]      # the values as they were, payload and sign
    res, rank, vout, mean = select_twice_and_check(v, 3)
    assert res[0] == 0x7F800000 and int(rank[17]) == 0                   # then +inf
    v2 = normal_values(4099).copy()
    v2[17] = np.inf
    res, rank, vout, mean = select_twice_and_check(v2, 5)
    assert np.isinf(mean[0]) and mean[0] > 0
    select_twice_and_check(v, 4099)                                       # -inf last


def test_select_optional_outputs_and_refusals():
    v = normal_values(257)
    dv = torch.from_numpy(v).to(DEV)
    res, rank, vout, mean = run_select(dv, 25, want=())
    assert rank is None and list(res) == tr.select_exact(v, 25)["result"]
    res, rank, vout, mean = run_select(dv, 25, want=("mean",))
    assert abs(float(mean[0]) - tr.select_exact(v, 25)["mean64"]) <= 1e-6
    ws = torch.empty(SELECT_WS, dtype=torch.uint8, device=DEV)
    assert lib().hdf_op_topk_select(ptr(dv), 257, 258, ptr(ws), ws.numel(), None, None, None, None, st()) == 1
    assert lib().hdf_last_error().startswith(b"topk:")


# ================================================================================================ the loss
def unaligned(x):
    """the same values in a contiguous view one element off a 16-byte boundary (the kernels' 1-voxel form)"""
    buf = torch.empty(x.numel() + 1, dtype=x.dtype, device=DEV)
    v = buf[1:].view(x.shape)
    v.copy_(x)
    assert v.data_ptr() % 16 != 0
    return v


def criterion(h, k, mean):
    from loss.cross_entropy import TopKLoss
    w = None if h["weight"] is None else h["weight"].float()
    return TopKLoss(weight=w, ignore_index=h["ignore"], k=k, reduction="topk" if mean else "mean")


def run_dropin(h, k, mean, off_alignment=False, shift=0, target=None):
    """forward and backward through the drop-in (through the node itself for a scale shift) -> (output, res, rank, dlogits,
    upstream gradient), on the host"""
    from hdf_rt.loss_fn import TopKVoxelCE, topk_workspace_views
    x = h["x"].to(DEV).to(TDT[h["dtype"]])
    t = (h["onehot"] if target is None else target).to(DEV)
    if off_alignment:
        x, t = unaligned(x), unaligned(t)
    x.requires_grad_(True)
    crit = criterion(h, k, mean)
    out = TopKVoxelCE.apply(crit._spec(t, shift), x) if shift else crit(x, t)
    assert out.dtype == torch.float32 and out.shape == (() if mean else (h["K"],))
    _lg, _tg, ws = out.grad_fn.saved_tensors
    res, rank = topk_workspace_views(ws, h["n"])
    res, rank = res.clone(), rank.clone()
    g = tr.upstream(h, mean).to(DEV)               # a device scalar (as a GradScaler hands it over) or a vector g[K]
    out.backward(g)
    torch.cuda.synchronize()
    assert x.grad.dtype == x.dtype
    return out.detach().cpu(), res.cpu(), rank.cpu(), x.grad.detach().float().cpu(), g.cpu()


def check_all(h, mean, out, res, rank, dl, g):
    tr.check_selection(h, rank)
    tr.check_own_selection(res.numpy(), rank.numpy())
    check_rounded(res, h["res64"], F32, h["acc_v"], "per-voxel loss")
    if mean:
        tr.check_mean(h, out)
        got64 = float(res[rank >= 0].double().mean())                      # the fp64 mean of its own values, rounded once
        assert abs(float(out) - got64) <= 2.0 ** -24 * abs(got64)
    else:
        tr.check_vector(h, out, res, rank)
    tr.check_grad(h, dl, rank, g, mean)


@pytest.mark.parametrize("mean", [False, True], ids=["vector", "topk"])
@pytest.mark.parametrize("case,dtype", PAIRS, ids=IDS)
def test_loss_and_gradient_against_the_restatement(case, dtype, mean):
    h = tr.held_to(case, dtype)
    check_all(h, mean, *run_dropin(h, tr.CASES[case][3], mean))


@pytest.mark.parametrize("mean", [False, True], ids=["vector", "topk"])
@pytest.mark.parametrize("case,dtype", [("small_odd", F32), ("c8_k1", BF16), ("flat2d", F16), ("multi_block", BF16)])
def test_views_one_element_off_16_byte_alignment(case, dtype, mean):
    h = tr.held_to(case, dtype)
    check_all(h, mean, *run_dropin(h, tr.CASES[case][3], mean, off_alignment=True))


def test_two_runs_are_bit_identical():
    h = tr.held_to("multi_block", BF16)
    a = run_dropin(h, 10, True)
    b = run_dropin(h, 10, True)
    for x, y in zip(a, b):
        assert x.numpy().tobytes() == y.numpy().tobytes()


def upsampled_target(h, shift):
    """a full-resolution one-hot target whose nearest down-sampling by 2^shift (index dst << shift) is the case's target;
    every other position holds another seeded class"""
    s = 1 << shift
    onehot = h["onehot"]
    c, sp = onehot.shape[1], tuple(onehot.shape[2:])
    lab = onehot.argmax(1)
    full = torch.randint(0, c, (onehot.shape[0],) + tuple(v * s for v in sp), generator=torch.Generator().manual_seed(31 + shift))
    full[(slice(None),) + (slice(None, None, s),) * len(sp)] = lab
    return torch.nn.functional.one_hot(full, c).movedim(-1, 1).float().contiguous()


@pytest.mark.parametrize("shift", [1, 2])
@pytest.mark.parametrize("case,dtype", [("small_odd", BF16), ("flat2d", F32), ("c8_k1", F16)])
def test_scale_shift_reads_the_full_resolution_target(case, dtype, shift):
    h = tr.held_to(case, dtype)
    t = upsampled_target(h, shift)
    assert torch.equal(torch.nn.functional.interpolate(t, size=tuple(h["onehot"].shape[2:])), h["onehot"])   # F.interpolate(nearest)
    for mean in (False, True):
        check_all(h, mean, *run_dropin(h, tr.CASES[case][3], mean, shift=shift, target=t))


def test_raw_entries():
    """the C entries themselves on one case, both forms: outputs, workspace contents, gradient"""
    from hdf_rt.loss_fn import topk_workspace_views
    case, dtype = "ignore0", BF16
    h = tr.held_to(case, dtype)
    x = h["x"].to(DEV).to(TDT[dtype]).contiguous()
    t = h["onehot"].to(DEV)
    cw = h["weight"].float().to(DEV)
    b, c, (d, hh, w) = x.shape[0], x.shape[1], x.shape[2:]
    nbytes = lib().hdf_loss_topk_workspace_bytes(b, d, hh, w)
    assert nbytes == SELECT_WS + 8 * h["n"]
    geom = (dtype, ptr(x), ptr(t), b, c, d, hh, w, 0, ptr(cw), h["ignore"], h["K"])
    for mean in (False, True):
        ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        out = torch.empty(1 if mean else h["K"], dtype=torch.float32, device=DEV)
        check(lib().hdf_loss_topk_forward(*geom, ptr(ws), nbytes, None if mean else ptr(out), ptr(out) if mean else None, st()), "fwd")
        g = tr.upstream(h, mean).to(DEV).reshape(-1)
        dl = torch.empty_like(x)
        check(lib().hdf_loss_topk_backward(*geom, ptr(ws), nbytes, None if mean else ptr(g), ptr(g) if mean else None, ptr(dl), st()),
              "bwd")
        torch.cuda.synchronize()
        res, rank = topk_workspace_views(ws, h["n"])
        check_all(h, mean, out.cpu()[0] if mean else out.cpu(), res.cpu(), rank.cpu(), dl.float().cpu(), g.cpu()[0] if mean else g.cpu())
    # refused on the device as on the host: nothing is launched, the output stays as it was
    out = torch.full((1,), -3.0, device=DEV)
    assert lib().hdf_loss_topk_forward(*geom[:-1], h["n"] + 1, ptr(ws), nbytes, None, ptr(out), st()) == 1
    assert lib().hdf_last_error().startswith(b"topk:") and float(out) == -3.0


def test_deep_supervision_over_four_scales():
    """DeepSuperloss(TopKLoss(reduction='topk')) = sum_i 2^-i TopK(out_i, target at index << i), K_i from each scale's voxel
    count, against the restated sum; every scale's gradient through the checks with its share 2^-i of the upstream scalar"""
    from loss.combine_loss import DeepSuperloss
    from loss.cross_entropy import TopKLoss
    shape, b, c, k, dtype = (24, 40, 40), 2, 4, 10, BF16
    gen = torch.Generator().manual_seed(77)
    lab = torch.randint(0, c, (b,) + shape, generator=gen)
    onehot = torch.nn.functional.one_hot(lab, c).movedim(-1, 1).float().contiguous()
    w = torch.tensor(tr.CLASS_WEIGHT[:c], dtype=torch.float64)
    hs = []
    for i in range(4):
        x = tr.rnd(torch.randn((b, c) + tuple(v >> i for v in shape), generator=gen) * 2.0, dtype)
        sub = onehot[(slice(None), slice(None)) + (slice(None, None, 1 << i),) * 3].contiguous()
        hs.append(tr.hold(x, sub, w, -100, k, dtype))
        assert int(hs[-1]["band"].sum()) <= tr.BAND_CAP
    outs = [h["x"].to(DEV).to(TDT[dtype]).requires_grad_(True) for h in hs]
    loss = DeepSuperloss(criterion=TopKLoss(weight=w.float(), k=k, reduction="topk"))(outs, onehot.to(DEV))
    parts = [n.saved_tensors[2] for n in _topk_nodes(loss.grad_fn)]
    (loss * 1024.0).backward()
    torch.cuda.synchronize()
    want = sum(h["mean64"] / (1 << i) for i, h in enumerate(hs))
    tol = sum((h["acc_v"] + 2.0 ** -24 * abs(h["mean64"])) / (1 << i) for i, h in enumerate(hs)) + 4 * 2.0 ** -24 * abs(want)
    got = float(loss.detach())
    assert loss.shape == () and abs(got - want) <= tol, (got, want, tol)
    from hdf_rt.loss_fn import topk_workspace_views
    assert len(parts) == 4
    by_n = {p.numel(): p for p in parts}
    for i, (h, o) in enumerate(zip(hs, outs)):
        ws = by_n[lib().hdf_loss_topk_workspace_bytes(b, *[v >> i for v in shape])]
        res, rank = topk_workspace_views(ws, h["n"])
        tr.check_selection(h, rank.cpu())
        tr.check_grad(h, o.grad.float().cpu(), rank.cpu(), torch.tensor(1024.0 / (1 << i)), True)


def _topk_nodes(fn, seen=None):
    """the TopKVoxelCE nodes of an autograd graph"""
    seen = set() if seen is None else seen
    if fn is None or fn in seen:
        return []
    seen.add(fn)
    found = [fn] if "TopKVoxelCE" in type(fn).__name__ else []
    for nxt, _ in fn.next_functions:
        found += _topk_nodes(nxt, seen)
    return found


@pytest.mark.parametrize("case", tr.GOLDEN_CASES)
def test_against_the_references_recorded_vector(case):
    gold = np.load(os.path.join(GOLDEN, "g12_topk_loss.npz"))
    h = tr.held_to(case, F32)
    assert np.array_equal(gold[case + "_logits"], h["x"].numpy())
    out, res, rank, dl, g = run_dropin(h, tr.CASES[case][3], False)
    assert out.numel() == int(gold[case + "_K"])
    ref = torch.from_numpy(gold[case + "_topk_desc"].copy()).double()
    # the reference's vector is an fp32 evaluation too: both lie within the fp32 allowance of the fp64 vector
    check_rounded(out.sort(descending=True).values, ref, F32, 2.0 * h["acc_v"] + 0.5 * 2.0 ** -23 * float(ref.abs().max()),
                  "vector against the golden")


def test_a_nan_logit_reaches_the_result():
    h = tr.held_to("c2", F32)
    from loss.cross_entropy import TopKLoss
    x = h["x"].clone()
    x[0, 1, 3, 4, 5] = float("nan")
    xd = x.to(DEV)
    out = TopKLoss(k=10)(xd, h["onehot"].to(DEV))
    assert out.numel() == h["K"] and int(torch.isnan(out).sum()) == 1          # counted as the largest: selected
    assert bool(torch.isnan(TopKLoss(k=10, reduction="topk")(xd, h["onehot"].to(DEV))))


def test_train_step_through_the_model():
    """HDenseFormer(2, 3, 16, (32, 32, 32), 8) with DeepSuperloss(TopKLoss(reduction='topk')): the loss and every gradient
    finite, and a repeat from the same state bit-identical in the loss and in the logit gradients the loss hands to the model
    (some of the model's own bias gradients are summed with fp32 atomics)"""
    from loss.combine_loss import DeepSuperloss
    from loss.cross_entropy import TopKLoss
    from models.HDenseFormer import HDenseFormer
    from oracle import detgen
    from oracle import hdf_oracle as orc
    cfg = (2, 3, 16, (32, 32, 32), 8)
    net = HDenseFormer(cfg[0], cfg[1], cfg[2], image_size=cfg[3], transformer_depth=cfg[4])
    net.load_state_dict(orc.det_model(*cfg))
    net = net.to(DEV).eval()
    x = torch.from_numpy(detgen.det_input(2, cfg[0], cfg[3], tag="g12_topk")).to(DEV)
    onehot = torch.from_numpy(detgen.one_hot(detgen.det_labels(2, cfg[1], cfg[3], tag="g12_topk"), cfg[1])).to(DEV)
    crit = DeepSuperloss(criterion=TopKLoss(weight=[0.5, 1.0, 2.0], k=10, reduction="topk"))
    runs = []
    for _ in range(2):
        for p in net.parameters():
            p.grad = None
        outs = net(x)
        for o in outs:
            o.retain_grad()
        loss = crit(outs, onehot)
        loss.backward()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(loss)) and float(loss.detach()) > 0
        assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in net.parameters())
        assert any(float(p.grad.abs().max()) > 0 for p in net.parameters())
        runs.append((loss.detach().clone(), [o.grad.clone() for o in outs]))
    assert torch.equal(runs[0][0], runs[1][0])
    assert all(torch.equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))
    # one voxel in ten of every scale carries a gradient
    for i, gl in enumerate(runs[0][1]):
        nz = int((gl.float().abs().sum(1) > 0).sum())
        assert nz <= tr.topk_count(gl[:, 0].numel(), 10) and nz >= 0.9 * tr.topk_count(gl[:, 0].numel(), 10), (i, nz)
