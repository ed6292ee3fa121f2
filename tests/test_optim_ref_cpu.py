"""CPU self-tests of tests/optim_ref.py: the check that test_gpu_optim_rounding.py applies to the optimizer kernels has
teeth.  On the data of every case of optim_ref.CASES torch's own fp32 optimizer (foreach=False), stepped once from the
same state, sits at or below HALF the bound; every applicable mutant of optim_ref.MUTANTS leaves elements of p beyond the
bound, in each group it concerns.  These are conditions on the cases' inputs (optim_ref.make), which were chosen so that
they hold.  Two mutants are invisible on some cases and are applied only where they are not: SGD's first step adding to
the old buffer needs a non-zero buffer at counter 0 (SGD.step1, SGD.plain.step1), and the bias corrections formed from a
power rounded to fp32 -- what the kernels did before this file -- differ from the right ones by 3.3e-6 at step 2, 3.1e-6
at step 3, 2.4e-6 at step 5 and less than 3e-7 from step 10, so it belongs to the cases of steps 2, 3 and 5.

The distance the ABI builds in is stated here too: betas arrive as fp32 (include/hdf.h), torch forms its corrections from
the Python doubles."""
import functools
import math

import pytest
import torch

import optim_ref as R

TEETH = [c for c in R.CASES if c["teeth"]]


@functools.lru_cache(maxsize=2)
def _ref(name):
    case = R.CASES[R.CASE_IDS.index(name)]
    d = R.make(case)
    args = (case["rule"], d["p"], d["g"], d["s1"], d["s2"], d["mask"] != 0, case["step"], case["h"])
    return case, d, args, R.step64(*args), R.bound(*args)


@functools.lru_cache(maxsize=None)
def _torch_ratio(name):
    case, d, args, ref, allow = _ref(name)
    got = R.torch_step(case, d)
    return max(R.ratio(a, b, c) for a, b, c in zip(got, ref, allow) if a is not None and b is not None)


@pytest.mark.parametrize("name", R.CASE_IDS)
def test_torch_fp32_step_is_within_half_the_bound(name):
    r = _torch_ratio(name)
    print("TORCH %s %.3f" % (name, r))
    assert r <= 0.5


def test_torch_worst_ratio_per_rule():
    """the figures in optim_ref's docstring (there against the unscaled running error: twice these)"""
    worst = {}
    for case in R.CASES:
        key = "hdf_adam_step" if case["entry"] == "adam" else R.RULE_NAME[case["rule"]]
        worst[key] = max(worst.get(key, 0.0), _torch_ratio(case["name"]))
    for key, r in worst.items():
        print("TORCH worst %s %.3f of the bound (K = %g)" % (key, r, R.K))
        assert r <= 0.5
    assert R.K <= 4.0


@pytest.mark.parametrize("name", [c["name"] for c in TEETH])
def test_every_applicable_mutant_is_caught(name):
    case, d, args, ref, allow = _ref(name)
    dec = d["mask"] != 0
    nonzero = bool((d["s1"] != 0).any())
    applied = 0
    for mutant in R.MUTANTS:
        if not R.applicable(mutant, case["rule"], case["step"], case["h"], nonzero):
            continue
        applied += 1
        beyond = ~((R.step64(*args, mutant=mutant)[0] - ref[0]).abs() <= allow[0])      # (a NaN is beyond)
        groups = R.groups_concerned(mutant, case["h"])
        parts = [beyond] if groups is None else [beyond[dec if grp else ~dec] for grp in groups]
        frac = [float(b.double().mean()) if b.numel() else float("nan") for b in parts]
        print("MUTANT %s %s beyond the bound: %s" % (name, mutant, " ".join("%.3f" % f for f in frac)))
        assert all(f > 0.0 for f in frac), (name, mutant, frac)
    assert applied >= 4


def test_every_mutant_is_applied_somewhere():
    for mutant in R.MUTANTS:
        where = [c["name"] for c in TEETH if R.applicable(mutant, c["rule"], c["step"], c["h"])]
        assert where, mutant
    rounded = [c["step"] for c in TEETH if R.applicable("bias_pow_rounded", c["rule"], c["step"], c["h"])]
    assert {2, 3, 5} == set(rounded)


def test_sgd_first_step_replaces_the_buffer_and_later_steps_do_not():
    case = R.CASES[R.CASE_IDS.index("SGD.step1")]
    d = R.make(case)
    assert bool((d["s1"] != 0).all())
    dec = d["mask"] != 0
    a = R.step64(R.SGD, d["p"], d["g"], d["s1"], None, dec, 1, case["h"])
    b = R.step64(R.SGD, d["p"], d["g"], -7.0 * d["s1"], None, dec, 1, case["h"])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    c = R.step64(R.SGD, d["p"], d["g"], -7.0 * d["s1"], None, dec, 2, case["h"])
    assert not torch.equal(a[0], c[0])


def test_two_tracked_steps_carry_the_error_of_the_first():
    """track() on its own output (the wrappers' two steps): the allowance of step 2 from a state that already carries an
    error is at least what the same step is allowed from an exact state, and at least the first step's error of p"""
    case = R.CASES[R.CASE_IDS.index("Adam.step2")]
    d = R.make(case)
    dec = d["mask"] != 0
    p, s1, s2 = R.track(R.ADAM, R.T(d["p"].double()), R.T(d["g"].double()), R.T(d["s1"].double()), R.T(d["s2"].double()),
                        dec, 2, case["h"])
    q = R.track(R.ADAM, p, R.T(d["g"].double()), s1, s2, dec, 3, case["h"])
    fresh = R.track(R.ADAM, R.T(p.v), R.T(d["g"].double()), R.T(s1.v), R.T(s2.v), dec, 3, case["h"])
    for carried, exact in zip(q, fresh):
        assert torch.equal(carried.v, exact.v) and bool((carried.e >= exact.e).all())
    assert bool((q[0].e >= p.e).all()) and bool((q[0].e > fresh[0].e).any())


def test_distance_of_the_fp32_betas_from_torchs_bias_correction():
    """sqrt(1 - b2^k) from 0.999f against the same from 0.999: d(b2) k b2^(k-1) / (2 (1 - b2^k)) with d(b2) = 1.29e-8.
    The sentence at hdf_optim_step / hdf_adam_step in include/hdf.h quotes these figures; a change of the ABI that moves
    them must change it."""
    want = {1: 6.4e-6, 100: 6.1e-6, 3000: 1.0e-6}
    b32 = R.f32(0.999)
    for k, figure in want.items():
        a, b = math.sqrt(1.0 - b32 ** k), math.sqrt(1.0 - 0.999 ** k)
        rel = abs(a - b) / b
        print("ABI sqrt(1 - b2^k), k = %d: %.12g (0.999f) %.12g (0.999), relative distance %.3e" % (k, a, b, rel))
        assert abs(rel - figure) <= 0.1 * figure
    hdr = open(R.HEADER).read()
    assert hdr.count("6.4e-6") >= 2 and hdr.count("1e-6 at step 3000") >= 2


def test_rounded_power_is_the_distance_the_issue_states():
    """bc2s as the kernels formed it (power rounded to fp32 first) against the same expression in double"""
    b1, b2 = R.f32(0.9), R.f32(0.999)
    rel = {}
    for k in (2, 3, 5, 10, 100):
        rel[k] = abs(R._bias(b1, b2, k, rounded=True)[1] - R._bias(b1, b2, k)[1]) / R._bias(b1, b2, k)[1]
        print("bc2s with the power rounded first, step %d: %.2e off (%.1f x 2^-24)" % (k, rel[k], rel[k] / R.U))
    assert abs(rel[2] - 3.3e-6) < 0.2e-6 and abs(rel[3] - 3.1e-6) < 0.2e-6 and abs(rel[5] - 2.4e-6) < 0.2e-6
    assert rel[10] < 3e-7 and rel[100] < 3e-7
