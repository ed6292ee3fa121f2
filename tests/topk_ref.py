"""CPU side of tests/test_gpu_topk_loss.py and tests/test_topk_ref_cpu.py: the seeded cases of TopKLoss, its restatement
(reference loss/cross_entropy.py:26-43) in fp64, in fp32 and on the softmax the kernels' fast intrinsics compute
(loss_ref.softmax_b), the exact select in numpy, the allowances and the guard band, and the checking functions the GPU test
applies to the kernels' output.  Nothing in here touches a GPU; every allowance is a property of the reference alone.

Restated, quirks included: TopKLoss(weight, ignore_index, k, reduction) hands reduce=False to torch.nn.CrossEntropyLoss, which
sets self.reduction = 'none' whatever `reduction` was, so forward returns torch.topk(res, K, sorted=False).values with res[v]
= weight[t_v] * nll_v (0 where t_v == ignore_index), t the arg-max of the one-hot target (first maximum), K = int(N * k / 100)
-- a K-vector in unspecified order.  Ours is in ascending voxel index; among values equal to the K-th largest the lowest index
is taken first; reduction='topk' is the mean of the vector."""
import functools
import math

import numpy as np
import torch

from hdf_rt._lib import BF16, F16, F32
from hip_util import check_rounded, rnd, ulp_of
from loss_ref import CLASS_WEIGHT, softmax_a, softmax_b

NAME = {F32: "f32", BF16: "bf16", F16: "f16"}
DTYPES = (F32, BF16, F16)

# name: (spatial shape, B, C, k, options).  mul: logits scale; weights: CLASS_WEIGHT[:C]; ignore: ignore_index
CASES = {
    "small_odd": ((8, 16, 24), 3, 3, 10, {}),
    "weighted_k50": ((8, 16, 24), 3, 3, 50, dict(weights=1)),
    "c2": ((8, 8, 16), 1, 2, 10, {}),
    "c8_k1": ((8, 8, 16), 1, 8, 1, dict(weights=1)),
    "saturated": ((8, 16, 16), 2, 4, 10, dict(mul=30.0)),
    "ignore0": ((16, 16, 16), 2, 4, 10, dict(weights=1, ignore=0)),
    "flat2d": ((40, 72), 2, 4, 10, {}),
    "multi_block": ((24, 40, 40), 2, 4, 10, {}),
}
SEED = {k: 4100 + 13 * i for i, k in enumerate(CASES)}
# recorded from the reference: the three smallest cases and `ignore0` -- not the fourth smallest (`flat2d` is), but the one
# that records the reference's ignore_index and class-weight behaviour
GOLDEN_CASES = ("c2", "c8_k1", "saturated", "ignore0")
BAND_CAP = 8                                                 # a case's guard band holds at most this many voxels


def case_weight(case, dt=torch.float64):
    c, o = CASES[case][2], CASES[case][4]
    return torch.tensor(CLASS_WEIGHT[:c], dtype=dt) if o.get("weights") else None


def case_ignore(case):
    return CASES[case][4].get("ignore", -100)


def topk_count(n, k):
    return int(n * k / 100)


@functools.lru_cache(maxsize=None)
def base_inputs(case):
    """(fp32 logits [B,C,*shape], class map int64 [B,*shape]) of the seed"""
    shape, b, c, _k, o = CASES[case]
    gen = torch.Generator().manual_seed(SEED[case])
    lab = torch.randint(0, c, (b,) + shape, generator=gen)
    x = torch.randn((b, c) + shape, generator=gen) * o.get("mul", 1.0)
    return x, lab


@functools.lru_cache(maxsize=4)
def inputs(case, dtype):
    """(logits rounded through the storage dtype, fp32 CPU; one-hot target fp32; class map)"""
    x, lab = base_inputs(case)
    c = CASES[case][2]
    onehot = torch.nn.functional.one_hot(lab, c).movedim(-1, 1).float().contiguous()
    return rnd(x, dtype), onehot, lab


# ------------------------------------------------------------------------------------------------ the restatement
def per_voxel(x, onehot, weight, ignore, dt=torch.float64, softmax=None):
    """res[v] = weight[t_v] * nll_v, 0 where t_v == ignore; flat in (b, d, h, w) order, dtype dt.  softmax: softmax_a /
    softmax_b of loss_ref (fp64 arithmetic on their p and logsumexp) instead of torch's log-sum-exp in dt"""
    t = onehot.argmax(1, keepdim=True)                       # first maximum
    if softmax is None:
        xd = x.to(dt)
        nll = torch.logsumexp(xd, 1, keepdim=True) - xd.gather(1, t)
    else:
        _p, lse = softmax(x)
        nll = (lse - x.double().gather(1, t)).to(dt)
    w = weight.to(dt)[t] if weight is not None else torch.ones_like(nll)
    res = torch.where(t == ignore, torch.zeros_like(nll), w * nll)
    return res.flatten()


def float_keys(v):
    """the order the select uses on fp32 values (numpy array): uint32 keys, NaN the largest, -0.0 below +0.0"""
    v = np.ascontiguousarray(v, dtype=np.float32)
    u = v.view(np.uint32)
    key = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))
    return np.where(np.isnan(v), np.uint32(0xFFFFFFFF), key).astype(np.uint32)


def key_bits(key):
    key = int(key)
    if key == 0xFFFFFFFF:
        return 0x7FC00000
    return key & 0x7FFFFFFF if key & 0x80000000 else (~key) & 0xFFFFFFFF


def select(order_keys, K, last_tie=False):
    """exact top-K of integer / float keys (any numpy array ordered by <): -> (threshold key, count above, ties taken, rank
    int32 [n], -1 = not selected).  Tie rule: lowest index first (last_tie: the planted defect, highest index first)"""
    n = order_keys.shape[0]
    assert 1 <= K <= n
    T = np.partition(order_keys, n - K)[n - K]
    above, tie = order_keys > T, order_keys == T
    gt = int(above.sum())
    ties = K - gt
    tie_idx = np.cumsum(tie) - 1
    if last_tie:
        tie_idx = int(tie.sum()) - 1 - tie_idx
    sel = above | (tie & (tie_idx < ties))
    rank = np.where(sel, np.cumsum(sel) - 1, -1).astype(np.int32)
    return T, gt, ties, rank


def select_exact(values, K, last_tie=False):
    """what hdf_op_topk_select must return for fp32 `values`: dict(result=[bits, above, ties, 0], rank, values_out, mean64)"""
    values = np.ascontiguousarray(values, dtype=np.float32)
    T, gt, ties, rank = select(float_keys(values), K, last_tie)
    out = values[rank >= 0]
    return dict(result=[key_bits(T), gt, ties, 0], rank=rank, values_out=out,
                mean64=math.fsum(out.astype(np.float64).tolist()) / K if not np.isnan(out).any() else float("nan"))


def gradient(x, onehot, weight, ignore, p, gvox):
    """closed form: d / d logits of sum_v gvox[v] * res[v] = gvox[v] * w[t_v] * (p_c - [c == t_v]), 0 on ignored voxels.
    p: softmax [B,C,...] fp64; gvox: flat per-voxel upstream gradient (0 on unselected voxels), fp64"""
    t = onehot.argmax(1, keepdim=True)
    oh = torch.zeros_like(p).scatter_(1, t, 1.0)
    w = weight.double()[t] if weight is not None else torch.ones_like(p[:, :1])
    k = torch.where(t == ignore, torch.zeros_like(w), w * gvox.double().view(t.shape))
    return torch.where(k != 0, k * (p - oh), torch.zeros_like(p))       # (an unselected voxel: +0, not 0 * negative = -0)


def gradient_autograd(x, onehot, weight, ignore, gvox, dt):
    """the same through autograd in dtype dt (F.cross_entropy as the reference calls it)"""
    z = x.to(dt).clone().requires_grad_(True)
    c = z.shape[1]
    t = onehot.argmax(1).reshape(-1)
    res = torch.nn.functional.cross_entropy(z.movedim(1, -1).reshape(-1, c), t, weight=None if weight is None else weight.to(dt),
                                            ignore_index=ignore, reduction="none")
    (res * gvox.to(dt)).sum().backward()
    return z.grad


def hold(x, onehot, w, ign, k, dtype, case=None):
    """everything a test holds one set of inputs to: res64, K, T64, the reference's selection (rank64), the vector and the
    mean in fp64, acc_v = 4 max|res32 - res64| + max|res(A) - res(B)|, the guard band |res64 - T64| <= 2 acc_v"""
    res64 = per_voxel(x, onehot, w, ign, torch.float64)
    res32 = per_voxel(x, onehot, w, ign, torch.float32)
    res_a = per_voxel(x, onehot, w, ign, torch.float64, softmax_a)
    res_b = per_voxel(x, onehot, w, ign, torch.float64, softmax_b)
    n = res64.numel()
    K = topk_count(n, k)
    T, gt, ties, rank = select(res64.numpy(), K)
    acc_v = 4.0 * float((res32.double() - res64).abs().max()) + float((res_a - res_b).abs().max())
    band = (res64 - float(T)).abs() <= 2.0 * acc_v
    vec = res64[torch.from_numpy(rank >= 0)]
    return dict(case=case, dtype=dtype, x=x, onehot=onehot, weight=w, ignore=ign, res64=res64, n=n, K=K, T64=float(T),
                rank64=torch.from_numpy(rank), vec64=vec, mean64=float(vec.mean()), acc_v=acc_v, band=band,
                ties=int((res64 == float(T)).sum()))


@functools.lru_cache(maxsize=4)
def held_to(case, dtype):
    """`hold` of a case of the table in one storage dtype"""
    x, onehot, _lab = inputs(case, dtype)
    return hold(x, onehot, case_weight(case), case_ignore(case), CASES[case][3], dtype, case)


def grad_held_to(h, gvox):
    """(grad64 [B,C,...], acc_g) for a flat per-voxel upstream gradient: acc_g = 4 max|grad32 - grad64| + max|grad(A) -
    grad(B)|, the fp32 / fp64 gradients by autograd, (A) / (B) the closed form on the two softmaxes"""
    x, onehot, w, ign = h["x"], h["onehot"], h["weight"], h["ignore"]
    g64 = gradient_autograd(x, onehot, w, ign, gvox, torch.float64)
    g32 = gradient_autograd(x, onehot, w, ign, gvox, torch.float32)
    ga = gradient(x, onehot, w, ign, softmax_a(x)[0], gvox)
    gb = gradient(x, onehot, w, ign, softmax_b(x)[0], gvox)
    return g64, 4.0 * float((g32.double() - g64).abs().max()) + float((ga - gb).abs().max())


def upstream(h, mean, seed=7):
    """the upstream gradient of a test: the scalar 1024 a GradScaler would hand to the 'topk' form, a seeded random g[K]
    for the vector form"""
    if mean:
        return torch.tensor(1024.0)
    return torch.rand(h["K"], generator=torch.Generator().manual_seed(seed)) + 0.5


def per_voxel_upstream(h, rank, g, mean):
    """gvox[v] = g[rank[v]] (vector form) or g / K ('topk'), 0 where rank[v] < 0"""
    rank = torch.as_tensor(rank).long()
    sel = rank >= 0
    gv = torch.zeros(h["n"], dtype=torch.float64)
    gv[sel] = (g.double() / h["K"]) if mean else g.double()[rank[sel]]
    return gv


# ------------------------------------------------------------------------------------------------ the checks
def sum_depth(n):
    """the most fp64 additions any one value passes through on its way into the kernels' sum: a thread of topk_write_kernel
    adds its block's tiles one after the other (chunk / 256 of them, chunk = the block's index range), a wave folds in 6
    butterfly steps, the four waves in 3 adds; topk_mean_kernel does the same over the block sums (ceil(blocks / 256) serial,
    6, 3).  The order is fixed, so the depth depends on n alone -- about 40 at 5 M values, not n."""
    chunk = -(-(-(-n // 1024)) // 256) * 256
    blocks = -(-n // chunk)
    return chunk // 256 + 6 + 3 + -(-blocks // 256) + 6 + 3


def check_select_exact(values, K, result, rank, values_out, mean, want=None):
    """hdf_op_topk_select against numpy, exact in every bit; mean_out within half an fp32 ulp of the fp64 mean.  The one
    addition to the half ulp is the error of the kernels' own fp64 sum against the exact sum (math.fsum): each value passes
    through at most sum_depth(n) additions of relative error 2^-53, plus the division: (depth + 1) 2^-53 mean|v|, some
    2^-47 of the mean of the magnitudes -- it matters only where the mean itself all but cancels."""
    want = want or select_exact(values, K)
    assert [int(r) for r in result] == want["result"], (list(result), want["result"])
    assert np.array_equal(np.asarray(rank, dtype=np.int32), want["rank"]), "rank"
    assert np.asarray(values_out, dtype=np.float32).tobytes() == want["values_out"].tobytes(), "values_out"
    m64 = want["mean64"]
    if math.isnan(m64):
        assert math.isnan(float(mean))
    elif math.isinf(m64):
        assert float(mean) == m64
    else:
        absmean = float(np.abs(want["values_out"].astype(np.float64)).sum()) / K
        tol = 0.5 * float(ulp_of(torch.tensor(m64, dtype=torch.float64), F32)) + (sum_depth(len(values)) + 1) * 2.0 ** -53 * absmean
        assert abs(float(mean) - m64) <= tol, (float(mean), m64, tol)


def check_selection(h, rank):
    """exactly K voxels selected, ranks 0..K-1 ascending in voxel index, and outside the guard band the reference's
    selection (any implementation within acc_v per voxel must make it there: order statistics are 1-Lipschitz in the
    sup norm)"""
    rank = torch.as_tensor(rank).long().flatten()
    assert rank.numel() == h["n"]
    sel = rank >= 0
    assert int(sel.sum()) == h["K"], "selected %d voxels, K = %d" % (int(sel.sum()), h["K"])
    assert torch.equal(rank[sel], torch.arange(h["K"])), "ranks are not 0..K-1 in voxel order"
    assert bool((rank[~sel] == -1).all())
    ref = h["rank64"] >= 0
    out = ~h["band"]
    assert torch.equal(sel[out], ref[out]), "%d voxels outside the guard band selected differently" % int((sel[out] != ref[out]).sum())


def check_own_selection(res_got, rank):
    """the implementation's rank is the exact selection, tie rule included, on its own per-voxel values"""
    res_got = np.asarray(res_got, dtype=np.float32)
    K = int((np.asarray(rank) >= 0).sum())
    assert np.array_equal(np.asarray(rank, dtype=np.int32), select(float_keys(res_got), K)[3]), "rank is not the exact selection"


def check_vector(h, vec, res_got, rank):
    """sorted, every element within 0.5 ulp(fp32) + acc_v of the sorted fp64 vector; as returned, res gathered by rank"""
    vec = torch.as_tensor(vec).float().flatten()
    assert vec.numel() == h["K"]
    check_rounded(vec.sort().values, h["vec64"].sort().values, F32, h["acc_v"], "top-k vector (sorted)")
    res_got, rank = torch.as_tensor(res_got).float().flatten(), torch.as_tensor(rank).long().flatten()
    assert torch.equal(vec, res_got[rank >= 0]), "the vector is not res in voxel order"
    check_rounded(res_got, h["res64"], F32, h["acc_v"], "per-voxel loss")


def check_mean(h, mean):
    tol = h["acc_v"] + 2.0 ** -24 * abs(h["mean64"])
    assert abs(float(mean) - h["mean64"]) <= tol, (float(mean), h["mean64"], tol)


def check_grad(h, dlogits, rank, g, mean):
    """every element of dlogits.  A voxel the implementation selected: check_rounded against the fp64 gradient with the
    upstream value of ITS rank; a voxel it did not select: exactly +0.  With check_selection this is: outside the band the
    reference's gradient or zero as the reference selects, inside the band either of the two -- never anything else."""
    rank = torch.as_tensor(rank).long().flatten()
    gvox = per_voxel_upstream(h, rank, g, mean)
    g64, acc_g = grad_held_to(h, gvox)
    dl = torch.as_tensor(dlogits).float()
    assert dl.shape == g64.shape
    sel = (rank >= 0).view((g64.shape[0], 1) + tuple(g64.shape[2:])).expand_as(g64)
    if sel.any():
        check_rounded(dl[sel], g64[sel], h["dtype"], acc_g, "dlogits on selected voxels")
    rest = dl[~sel]
    assert bool((rest == 0).all()) and not bool(torch.signbit(rest).any()), \
        "%d gradient elements of unselected voxels are not +0" % int(((rest != 0) | torch.signbit(rest)).sum())
