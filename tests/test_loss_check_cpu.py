"""Self-tests, on the CPU alone, of what tests/test_gpu_loss_rounding.py and tests/test_gpu_metrics_inference.py hold the
loss, metric and inference-tail kernels to (pattern: tests/test_rounding_check_cpu.py).  The "kernel output" here is the
fp64 reference rounded once into the storage type, with one planted defect; each defect must be rejected and the
unfaulted rounding accepted:
  (a) a 16-bit store of dlogits that truncates instead of rounding;
  (b) float16 subnormals flushed to zero (the unscaled float16 gradient past the cap is subnormal);
  (c) the voxels past the first grid trip left out of the Dice and CE sums -- the loss bound rejects it on cap_vec4;
  (d) the last voxel of each row of scale 1 taking its target from the neighbouring voxel;
  (e) one confusion-matrix count moved to the neighbouring class.
Also here: the closed-form logit gradient of tests/loss_ref.py (needed to swap the softmax for the one the kernels' fast
intrinsics compute) pinned to the oracle's fp64 autograd -- never to a kernel; the fp32 / fp64 restatement of the focal
losses pinned to tests/test_focal_loss_cpu.py `restated`; and the two conditions that the GPU tests put on their own
reference data (share of elements in the rounding-bias statistic, share of near-ties excluded from the vote), with the
reason why the rounding bias is measured against that of the correctly rounded reference (hip_util.rne_bias)."""
import pytest
import torch

import loss_ref as lr
import metrics_ref as mr
from hdf_rt._lib import BF16, F16, F32
from hip_util import check_rounded, check_rounding_bias, rne_bias, rounding_excess, signed_rounding_bias
from test_focal_loss_cpu import restated
from test_rounding_check_cpu import _truncate


@pytest.mark.parametrize("case", ["small_odd", "c2", "c8", "absent", "saturated", "cap_2d"])
def test_closed_form_gradient_is_the_oracles_autograd(case):
    outs, onehot = lr.inputs(case, BF16)
    for form in lr.FORMS:
        for gout in (1.0, 0.37):
            l64, g64 = lr.reference(outs, onehot, form, torch.float64, gout)
            (la, ga), _ = lr.closed_both(case, BF16, form, gout)
            assert abs(la - l64) <= 1e-12 * abs(l64), (form, la, l64)
            for i, (a, b) in enumerate(zip(ga, g64)):
                assert float((a - b).abs().max()) <= 1e-12 * float(b.abs().max()), (form, i)


def test_softmax_b_is_a_softmax_to_fp32_accuracy():
    outs, _ = lr.inputs("small_odd", F32)
    (pa, la), (pb, lb) = lr.softmax_a(outs[0]), lr.softmax_b(outs[0])
    assert 0 < float((pa - pb).abs().max()) < 1e-6 and float((la - lb).abs().max()) < 1e-6


@pytest.mark.parametrize("kind", ["focal", "flpd"])
def test_focal_restatement_in_fp64_is_restated(kind):
    outs, onehot = lr.inputs("c2", BF16)
    spec = lr.focal_spec(kind, 2)
    l0, g0 = restated(outs, onehot, spec)
    l1, g1 = lr.restated_in(outs, onehot, spec, torch.float64)
    assert l0 == l1 and all(torch.equal(a, b) for a, b in zip(g0, g1))
    l2, g2 = lr.restated_in(outs, onehot, spec, torch.float32)
    assert abs(l2 - l0) < 1e-4 * abs(l0) and all(float((a.double() - b).abs().max()) < 1e-4 * float(b.abs().max())
                                                 for a, b in zip(g2, g0))


@pytest.mark.parametrize("dtype", [BF16, F16])
def test_rounded_reference_is_accepted_and_a_truncating_store_is_rejected(dtype):
    # float16 with GradScaler's initial scale: unscaled, 1 / 270 336 voxels is subnormal throughout (see below)
    h = lr.held_to("cap_vec1", dtype, lr.DEFAULT, 65536.0 if dtype == F16 else 1.0)
    for g, acc in zip(h["grads64"], h["acc"]):
        assert check_rounded(lr.to_storage(g, dtype), g, dtype, acc) <= 1.0
        assert lr.bias_conditions_met(g, dtype)
        check_rounding_bias(lr.to_storage(g, dtype), g, dtype, expected=rne_bias(g, dtype))
        trunc = _truncate(g.float(), dtype)
        with pytest.raises(AssertionError, match="outside the bound"):
            check_rounded(trunc, g, dtype, acc)
        with pytest.raises(AssertionError, match="signed rounding bias"):
            check_rounding_bias(trunc, g, dtype, expected=rne_bias(g, dtype))
        assert signed_rounding_bias(trunc, g, dtype)[0] < -0.45


def test_the_rounded_reference_has_a_bias_of_its_own_on_clustered_values():
    """why the GPU tests measure the bias against hip_util.rne_bias: the two-class softmax of bf16 logits takes clustered
    values, and the reference rounded to nearest-even -- no kernel anywhere -- is outside 6 sigma of zero"""
    h = lr.held_to("cap_2d", BF16, lr.DEFAULT)
    g = h["grads64"][0]
    assert lr.bias_conditions_met(g, BF16)
    own = rne_bias(g, BF16)
    assert 0.005 < abs(own) < 0.05
    with pytest.raises(AssertionError, match="signed rounding bias"):
        check_rounding_bias(lr.to_storage(g, BF16), g, BF16)
    check_rounding_bias(lr.to_storage(g, BF16), g, BF16, expected=own)
    with pytest.raises(AssertionError, match="signed rounding bias"):
        check_rounding_bias(_truncate(g.float(), BF16), g, BF16, expected=own)


def test_flushed_float16_subnormals_are_rejected():
    h = lr.held_to("cap_vec1", F16, lr.DEFAULT)
    g, acc = h["grads64"][0], h["acc"][0]
    assert float(g.abs().max()) < 2.0 ** -14                        # 1 / 270 336 voxels: every element is subnormal
    good = lr.to_storage(g, F16)
    assert check_rounded(good, g, F16, acc) <= 1.0
    # a handful of ulp each: the correctly rounded reference shows a signed bias of its own, which the check allows for
    with pytest.raises(AssertionError, match="signed rounding bias"):
        check_rounding_bias(good, g, F16)
    check_rounding_bias(good, g, F16, expected=rne_bias(g, F16))
    flushed = torch.where(good.abs() < 2.0 ** -14, torch.zeros_like(good), good)
    with pytest.raises(AssertionError, match="outside the bound"):
        check_rounded(flushed, g, F16, acc)
    assert float((rounding_excess(flushed, g, F16, acc) > 1).double().mean()) > 0.5
    with pytest.raises(AssertionError, match="signed rounding bias"):
        check_rounding_bias(flushed, g, F16, expected=rne_bias(g, F16))


@pytest.fixture(scope="module")
def cap_vec4_bf16():
    return lr.held_to("cap_vec4", BF16, lr.DEFAULT)


def test_a_loss_that_stops_after_the_first_grid_trip_is_rejected(cap_vec4_bf16):
    """(c): scale 0 of cap_vec4 has 1 105 920 voxels per sample, the first trip of 1024 blocks x 256 threads x 4 covers
    1 048 576; the sums of a kernel whose loop does not come round again miss the rest"""
    h = cap_vec4_bf16
    outs, onehot = lr.inputs("cap_vec4", BF16)
    la, _ = h["closed"]
    assert abs(la - h["loss64"]) <= h["loss_tol"]                   # the unfaulted loss is accepted
    cut = 1024 * 256 * 4
    x0 = outs[0].flatten(2)[:, :, :cut]
    t0 = onehot.flatten(2)[:, :, :cut]
    p, lse = lr.softmax_a(x0)
    t, n, c = t0.double(), x0.shape[0], x0.shape[1]
    # CE is a mean over all voxels: the sum that stops early is still divided by the full count
    ce = (lse - x0.double().gather(1, t.argmax(1, keepdim=True))).sum() / (n * outs[0][0, 0].numel())
    inter, union = (p * t).sum(2), (p + t).sum(2)
    part = float(ce + (1.0 - (2.0 * inter + lr.SMOOTH) / (union + lr.SMOOTH)).mean(0)[1:].sum() / (c - 1))
    full, _ = lr.closed_form(outs[0], onehot, *lr.softmax_a(outs[0]), lr.DEFAULT, 0)
    faulty = la - full + part
    assert abs(faulty - h["loss64"]) > h["loss_tol"], (faulty, h["loss64"], h["loss_tol"])
    assert abs(faulty - h["loss64"]) < 0.1 * abs(h["loss64"])       # ... and is not a gross error


def test_cap_vec4_reference_meets_the_bias_conditions(cap_vec4_bf16):
    for g in cap_vec4_bf16["grads64"]:
        _, used, n = signed_rounding_bias(g, g, BF16)
        assert used >= 10000 and used >= 0.97 * n, (used, n)
        assert lr.bias_conditions_met(g, BF16) and lr.bias_conditions_met(g, F16)
    h = lr.held_to("cap_vec1", BF16, lr.DEFAULT)
    assert all(lr.bias_conditions_met(g, BF16) for g in h["grads64"])
    h = lr.held_to("saturated", BF16, lr.DEFAULT)                   # ... and a case that does not: no bias check there
    assert not any(lr.bias_conditions_met(g, BF16) for g in h["grads64"])


@pytest.mark.parametrize("dtype", [F32, BF16, F16])
def test_a_row_end_that_reads_the_neighbours_target_is_rejected(dtype):
    """(d): at scale 1 the target of voxel x is the full-resolution voxel 2 x; the defect reads 2 x - 1 on the last
    voxel of each row -- one voxel in 12 of small_odd's scale 1, invisible to max error / max reference at 10 %"""
    h = lr.held_to("small_odd", dtype, lr.DEFAULT)
    outs, onehot = lr.inputs("small_odd", dtype)
    t = lr.subsample(onehot, 1).clone()
    t[..., -1] = onehot[:, :, ::2, ::2, -3]
    assert not torch.equal(t, lr.subsample(onehot, 1))
    _, bad = lr.closed_form(outs[1], t, *lr.softmax_a(outs[1]), lr.DEFAULT, 1, sums_of=lr.subsample(onehot, 1))
    g, acc = h["grads64"][1], h["acc"][1]
    assert check_rounded(lr.to_storage(g, dtype), g, dtype, acc) <= 1.0
    with pytest.raises(AssertionError, match="outside the bound"):
        check_rounded(lr.to_storage(bad, dtype), g, dtype, acc)
    ratio = rounding_excess(lr.to_storage(bad, dtype), g, dtype, acc)
    assert bool((ratio[..., :-1] <= 1).all()) and bool((ratio[..., -1] > 1).any())


def test_a_count_moved_to_the_neighbouring_class_is_rejected():
    logits, lab = mr.metric_inputs(1, 5, 257, 31, 0.25)
    pred = mr.first_argmax(logits.to(torch.bfloat16).float())
    conf = mr.confusion_of(lab, pred, 5)
    assert int(conf.sum()) == 257 and torch.equal(conf, mr.confusion_of(lab, pred, 5))
    moved = conf.clone()
    t, p = (int(v) for v in torch.nonzero(conf)[0])
    moved[t, p] -= 1
    moved[t, (p + 1) % 5] += 1
    assert int(moved.sum()) == int(conf.sum()) and not torch.equal(moved, conf)
    cnt = mr.dice_counts_of(lab, pred, 5)
    assert torch.equal(cnt[0, :, 0], conf.diagonal()) and torch.equal(cnt[0, :, 1], conf.sum(0))
    assert torch.equal(cnt[0, :, 2], conf.sum(1)) and not torch.equal(cnt[0, :, 1], moved.sum(0))


def test_first_argmax_takes_the_first_of_tied_maxima():
    x = torch.tensor([[[1.0, 2.0, 0.5], [1.0, 2.0, 0.5], [0.0, 2.0, 0.5]]])       # [1, 3 classes, 3 voxels]
    assert mr.first_argmax(x).tolist() == [[0, 0, 0]]
    logits, _ = mr.metric_inputs(3, 5, 4096, 32, 0.25)
    r = logits.to(torch.bfloat16).float()
    top2 = r.topk(2, 1).values
    assert float((top2[:, 0] == top2[:, 1]).double().mean()) > 0.001             # exact ties are common at 16 bits
    assert torch.equal(mr.first_argmax(r), r.argmax(1))                          # torch.argmax's documented rule


@pytest.mark.parametrize("c", [2, 8])
def test_finalize_inputs_keep_the_exclusion_under_a_tenth_of_a_percent(c):
    psum, cnt, tied = mr.finalize_inputs(c)
    label, excluded = mr.finalize_reference(psum, cnt)
    assert float(excluded.double().mean()) <= 1e-3
    assert 0.15 < float((cnt == 0).double().mean()) < 0.25 and 0.03 < float(tied.double().mean()) < 0.07
    assert bool((label[cnt == 0] == 0).all()) and int(label.max()) == c - 1
    both = tied & (cnt > 0)
    assert bool((psum.double().max(0).values[both] == psum.double().topk(2, 0).values[1][both]).all())
    assert bool((label[both] < c - 1).all())                       # a tie at the top goes to the first of the two
