"""tests/quantile_ref.py, the restatement the GPU test of hdf_cc_quantiles compares with, held to np.sort at the stated
ranks, to live np.quantile and scipy.ndimage.median within bounds derived from their own arithmetic, to a plain loop on
inputs with ties, and to seven planted defects that its comparison must name.  Then what can be checked of the entry
without a GPU: every refusal comes before a launch, and the Python layer exports the feature.

The bound against np.quantile.  numpy forms the virtual index as n q + (1 - q) - 1 (three roundings of numbers up to n, so
it is within about 3 u n of h) and interpolates with a two-branch lerp; the restatement rounds h once.  A shift of the
index by e moves the piecewise linear interpolant by at most e g, g the largest gap between neighbours among s_{lo-1}, s_lo,
s_hi, s_{hi+1} (at an integer h numpy may take the interval on the other side: the interpolant is continuous there).  The
roundings of either lerp are a few u max|x|.  Together: 4 u n g + 4 u max|x|, u = 2^-53.
The bound against scipy's median: (s_lo + s_hi) / 2 in one order or another, each within a rounding or two of the exact
mean of two fp32 values: 2 u (|m| + |s_lo| + |s_hi|); exact where the values are small integers."""
import ctypes as C
import importlib.util
import os
from fractions import Fraction

import numpy as np
import pytest
from scipy import ndimage as ndi

import measure_ref as mr
import quantile_ref as qr
from conftest import ROOT

U = 2.0 ** -53
TEN = (0.0, 1.0, 0.5, 1.0 / 3.0, 0.95, 0.1, 0.9, 0.25, 0.75, 0.999)


def _as_got(want):
    return {k: np.array(want[k], copy=True) for k in ("count", "values", "result")}


def _ids_of(shape, key):
    return mr.labelled(shape, key[1], key[2])[0] if key[0] == "label" else mr.special_ids(shape, key[1])[0]


# ------------------------------------------------------------------------------------------------ np.sort at the ranks
@pytest.mark.parametrize("kind", ["signed", "levels", "zeros_denormals", "ints"])
@pytest.mark.parametrize("ids_key", [("label", "rand20", 26), ("special", "classes"), ("special", "gaps"), ("special", "tiny")],
                         ids=lambda k: "-".join(map(str, k)))
def test_the_order_statistics_are_np_sort_at_the_stated_ranks(kind, ids_key):
    shape = (5, 17, 33)
    ids = _ids_of(shape, ids_key)
    img = mr.image(kind, shape, 2)
    cap = int(max(ids.max(), 1)) + 2
    want = qr.quantiles(ids, img, qr.LEVELS16, cap)
    assert want["result"] == mr.measure(ids, img, cap)["result"]
    seen = 0
    for i in range(1, cap + 1):
        m = ids == i
        n = int(m.sum())
        assert want["count"][i - 1] == n
        if n == 0:
            assert not want["values"][:, i - 1].view(np.int64).any()
            continue
        seen += 1
        for c in range(2):
            s = np.sort(img[c][m] + np.float32(0.0)).astype(np.float64)
            for k, q in enumerate(qr.LEVELS16):
                h = q * float(n - 1)
                lo = int(np.floor(h))
                hi = lo + (h - lo > 0)
                assert 0 <= lo <= hi <= n - 1 and hi - lo <= 1
                got = want["values"][c, i - 1, k]
                assert got[0].tobytes() == s[lo].tobytes() and got[1].tobytes() == s[hi].tobytes(), (i, c, q)
                assert got[0] <= got[2] <= got[1]
                if q == 0.0:
                    assert got[2] == s[0] and got[0] == got[1] == s[0]
                if q == 1.0:
                    assert got[2] == s[-1] and got[0] == got[1] == s[-1]
    assert seen >= (1 if ids_key[1] == "tiny" else 3)
    # q = 0 and q = 1 are measure_ref's min and max in every bit
    ext = mr.measure(ids, img, cap)["stats"]
    k0, k1 = qr.LEVELS16.index(0.0), qr.LEVELS16.index(1.0)
    assert want["values"][:, :, k0, 2].tobytes() == np.ascontiguousarray(ext[..., 3]).tobytes()
    assert want["values"][:, :, k1, 2].tobytes() == np.ascontiguousarray(ext[..., 4]).tobytes()


# ------------------------------------------------------------------------------------------------ live numpy and scipy
def _trial_values(rng, n, dist):
    if dist == 0:
        return rng.standard_normal(n).astype(np.float32)
    if dist == 1:
        return rng.integers(-20, 60, n).astype(np.float32)
    if dist == 2:                                                # 40 decades of exponent, both signs
        return (rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-20.0, 20.0, n)).astype(np.float32)
    return rng.random(n, dtype=np.float32)


def test_the_interpolant_against_live_np_quantile_and_scipy_median():
    rng = np.random.default_rng(11)
    worst, medians, exact = 0.0, 0, 0
    for case in range(2000):
        n = int(rng.integers(1, 400))
        dist = case % 4
        x = _trial_values(rng, n, dist)
        ids = np.ones((1, 1, n), np.int32)
        want = qr.quantiles(ids, x.reshape(1, 1, 1, n), TEN, 1)
        s = np.sort(x.astype(np.float64))
        live = np.quantile(x.astype(np.float64), TEN)
        for k, q in enumerate(TEN):
            lo, hi = (int(v[0]) for v in qr.ranks(np.asarray([n]), q)[:2])
            around = s[max(lo - 1, 0): min(hi + 1, n - 1) + 1]
            g = float(np.max(np.diff(around))) if around.size > 1 else 0.0
            bound = 4 * U * n * g + 4 * U * float(np.max(np.abs(x)))
            err = abs(float(want["values"][0, 0, k, 2]) - float(live[k]))
            assert err <= bound, (case, n, q, err, bound)
            if err > 0:
                worst = max(worst, err / bound)
        if case % 10 == 0:                                       # scipy's median of the same component
            m = float(ndi.median(x.astype(np.float64), ids[0, 0], 1))
            lo_v, hi_v, mid = (float(v) for v in want["values"][0, 0, 2])
            assert abs(mid - m) <= 2 * U * (abs(m) + abs(lo_v) + abs(hi_v)), (case, n, mid, m)
            medians += 1
            exact += mid == m
            if dist == 1:
                assert mid == m, (case, n, mid, m)
    print("np.quantile: worst error / bound = %.3g; scipy medians bit-equal: %d of %d" % (worst, exact, medians))
    assert medians == 200


def test_the_median_of_a_labelled_volume_is_scipys():
    shape = (5, 17, 33)
    ids = mr.special_ids(shape, "classes")[0]
    img = mr.image("ints", shape, 1)
    want = qr.quantiles(ids, img, (0.5,), 3)
    sci = np.asarray(ndi.median(img[0].astype(np.float64), ids, [1, 2, 3]))
    assert want["values"][0, :, 0, 2].tobytes() == sci.astype(np.float64).tobytes()


# ------------------------------------------------------------------------------------------------ ties: a plain loop
@pytest.mark.parametrize("kind", ["levels", "constant", "zeros_denormals"])
def test_the_restatement_against_a_plain_loop_on_ties(kind):
    shape = (4, 7, 9)
    ids = mr.special_ids(shape, "classes")[0]
    img = mr.image(kind, shape, 2)
    levels = (0.5, 0.0, 1.0, 0.3, 0.5)
    want = qr.quantiles(ids, img, levels, 5)
    for c in range(2):
        for i in range(1, 6):
            mine = []
            for z in range(shape[0]):
                for y in range(shape[1]):
                    for x in range(shape[2]):
                        if ids[z, y, x] == i:
                            v = float(img[c, z, y, x])
                            mine.append(0.0 if v == 0.0 else v)
            n = len(mine)
            assert want["count"][i - 1] == n
            if n == 0:
                assert not want["values"][c, i - 1].any()
                continue
            mine.sort()
            for k, q in enumerate(levels):
                h = q * float(n - 1)
                lo = int(h // 1)
                frac = h - lo
                hi = lo + (1 if frac > 0 else 0)
                third = mine[lo] + frac * (mine[hi] - mine[lo])
                row = want["values"][c, i - 1, k]
                assert row.tobytes() == np.asarray([mine[lo], mine[hi], third]).tobytes(), (c, i, q)
    if kind == "zeros_denormals":
        assert (img.view(np.uint32) == 0x80000000).any()
        v = want["values"]
        assert (v == 0).any() and not np.signbit(v[v == 0]).any()


# ------------------------------------------------------------------------------------------------ planted defects
def order_of(x):
    """numpy's copy of the device's key: the bits of a float32 as a uint32 that orders like the value, -0 as +0"""
    bits = np.ascontiguousarray(x, np.float32).view(np.uint32).copy()
    bits[bits == 0x80000000] = 0
    return np.where(bits >> 31 != 0, ~bits, bits ^ np.uint32(0x80000000)).astype(np.uint32)


def value_of(key):
    key = np.asarray(key, np.uint32)
    return np.where(key >> 31 != 0, key ^ np.uint32(0x80000000), ~key).astype(np.uint32).view(np.float32)


def radix_select(keys, rank, strict=True):
    """the key of rank `rank` among keys by four rounds of 8 bits from the top, as the device does it.  strict=False plants
    `<=` for `<` at the bin boundary of the cumulative scan."""
    live, r, out = keys, int(rank), 0
    for shift in (24, 16, 8, 0):
        digits = (live >> np.uint32(shift)) & np.uint32(255)
        cnt = np.bincount(digits.astype(np.int64), minlength=256)
        incl = np.cumsum(cnt)
        hit = np.flatnonzero(r < incl if strict else r <= incl)
        d = int(hit[0]) if hit.size else 255
        r -= int(incl[d] - cnt[d])
        out = (out << 8) | d
        live = live[digits == d]
    return out


def _variant(ids, image, q, cap, defect=None):
    """the definition as a loop per id with one defect planted (None: none)"""
    ids = np.where(ids < 0, 0, ids)
    if defect == "fold":
        ids = np.minimum(ids, cap)
    C_ = image.shape[0]
    count = np.zeros(cap, np.int64)
    values = np.zeros((C_, cap, len(q), 3))
    flat = ids.ravel()
    result = [int(flat.max()), int((flat > 0).sum()), int(((flat > 0) & (flat <= cap)).sum()), 0]
    for i in range(1, cap + 1):
        where = np.flatnonzero(flat == i)
        n = where.size
        count[i - 1] = n
        if n == 0:
            continue
        for c in range(C_):
            x = image[c].ravel()[where]
            if defect != "minus_zero":
                x = x + np.float32(0.0)
            if defect == "signed_keys":
                s = x[np.argsort(x.view(np.int32), kind="stable")]
            else:
                s = np.sort(x)
                if defect == "minus_zero":                       # -0 below +0, as the raw keys order them
                    s = x[np.lexsort((~np.signbit(x), x))]
            keys = order_of(x)
            for k, level in enumerate(q):
                h = level * float(n) if defect == "q_n" else level * float(n - 1)
                h = min(h, float(n - 1))
                lo = int(np.floor(h))
                frac = h - lo
                hi = lo + (1 if (frac > 0 or defect == "hi_always") else 0)
                hi = min(hi, n - 1)
                if defect == "scan":
                    s_lo = float(value_of(radix_select(keys, lo, strict=False)))
                    s_hi = float(value_of(radix_select(keys, hi, strict=False)))
                elif defect == "radix":                          # no defect: the select itself
                    s_lo, s_hi = float(value_of(radix_select(keys, lo))), float(value_of(radix_select(keys, hi)))
                else:
                    s_lo, s_hi = float(s[lo]), float(s[hi])
                if defect == "fp32":
                    third = float(np.float32(s_lo) + np.float32(frac) * (np.float32(s_hi) - np.float32(s_lo)))
                elif defect == "fused":                          # fma(frac, fl(s_hi - s_lo), s_lo): one rounding for two
                    third = float(Fraction(s_lo) + Fraction(frac) * Fraction(s_hi - s_lo))
                else:
                    third = s_lo + frac * (s_hi - s_lo)
                values[c, i - 1, k] = s_lo, s_hi, third
    return dict(count=count, values=values, result=result)


def test_planted_defects_are_named():
    shape = (6, 11, 23)
    classes = mr.special_ids(shape, "classes")[0]
    signed, zeros = mr.image("signed", shape, 1), mr.image("zeros_denormals", shape, 1)
    levels = (0.5, 0.0, 1.0, 1.0 / 3.0, 0.95, 0.25)
    want = qr.quantiles(classes, signed, levels, 3)
    # nothing planted: nothing named -- by the loop and by the radix select, whose scan is the device's
    assert qr.mismatches(_variant(classes, signed, levels, 3), want) == []
    assert qr.mismatches(_variant(classes, signed, levels, 3, "radix"), want) == []
    assert qr.mismatches(_variant(classes, zeros, levels, 3, "radix"), qr.quantiles(classes, zeros, levels, 3)) == []
    assert qr.mismatches(_as_got(want), want) == []

    # 1. the rank from q n instead of q (n - 1)
    bad = qr.mismatches(_variant(classes, signed, levels, 3, "q_n"), want)
    assert "lower" in bad and "value" in bad and "count" not in bad
    # 2. hi = lo + 1 where frac = 0: an odd count, so the median has frac = 0
    odd = np.array(classes)
    if int((odd == 1).sum()) % 2 == 0:
        odd.ravel()[np.flatnonzero(odd.ravel() == 1)[0]] = 0
    want_odd = qr.quantiles(odd, signed, (0.5,), 3)
    assert int(want_odd["count"][0]) % 2 == 1
    assert qr.mismatches(_variant(odd, signed, (0.5,), 3, "hi_always"), want_odd) == ["upper"]
    # 3. keys compared as signed integers: the negatives come out reversed
    bad = qr.mismatches(_variant(classes, signed, levels, 3, "signed_keys"), want)
    assert "lower" in bad and "upper" in bad and "value" in bad
    # 4. -0 kept apart from +0: among zeros and denormals of both signs some rank falls on a -0
    want_z = qr.quantiles(classes, zeros, qr.LEVELS16, 3)
    bad = qr.mismatches(_variant(classes, zeros, qr.LEVELS16, 3, "minus_zero"), want_z)
    assert bad and set(bad) <= {"lower", "upper", "value"}
    # 5. ids above the capacity folded into the last row
    want2 = qr.quantiles(classes, signed, levels, 2)
    bad = qr.mismatches(_variant(classes, signed, levels, 2, "fold"), want2)
    assert "count" in bad and "result" in bad and "value" in bad
    # 6. the interpolation in fp32, and with one fused rounding
    # (the fused form differs from the three roundings only where the product's rounding tips the sum's: sixty ids, sixteen
    # levels, so that some row shows it)
    many = np.random.default_rng(3).integers(0, 61, shape).astype(np.int32)
    want_many = qr.quantiles(many, signed, qr.LEVELS16, 60)
    assert qr.mismatches(_variant(many, signed, qr.LEVELS16, 60), want_many) == []
    assert qr.mismatches(_variant(many, signed, qr.LEVELS16, 60, "fp32"), want_many) == ["value"]
    assert qr.mismatches(_variant(many, signed, qr.LEVELS16, 60, "fused"), want_many) == ["value"]
    # 7. `<=` for `<` at a bin boundary of the cumulative scan: the rank that is the first of its bin lands in the bin before
    bad = qr.mismatches(_variant(classes, signed, levels, 3, "scan"), want)
    assert "lower" in bad and "count" not in bad
    # a row of an absent id that is not zero bytes
    gaps, top = mr.special_ids((4, 10, 25), "gaps")
    want_g = qr.quantiles(gaps, mr.image("uniform", (4, 10, 25), 2), (0.5, 0.9), top + 3)
    assert (want_g["count"] == 0).sum() >= 30
    got = _as_got(want_g)
    got["values"][1, 0, 1, 2] = -0.0
    assert qr.mismatches(got, want_g) == ["value", "absent rows"]
    got = _as_got(want_g)
    got["count"][0] = 1
    assert qr.mismatches(got, want_g) == ["count", "absent rows"]


# ------------------------------------------------------------------------------------------------ the entry, without a GPU
@pytest.fixture(scope="module")
def lib():
    from hdf_rt import _lib
    if not os.path.exists(_lib.LIB_PATH):
        spec = importlib.util.spec_from_file_location("hdf_build", os.path.join(ROOT, "h-denseformer_amd", "build.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mod.build(verbose=False)
    return _lib.lib()


def test_the_feature_is_exported():
    import hdf_rt
    from hdf_rt import _lib
    assert callable(hdf_rt.region_quantiles) and callable(hdf_rt.region_order_stats) and callable(hdf_rt.region_median)
    assert "hdf_cc_quantiles" in _lib.EXPORTS and "hdf_cc_quantiles_workspace_bytes" in _lib.EXPORTS
    assert {"region_quantiles", "region_order_stats", "region_median"} <= set(dir(hdf_rt))


def test_the_workspace_size(lib):
    for c, cap, nq in ((0, 16, 1), (9, 16, 1), (-1, 16, 1), (1, 0, 1), (1, 65537, 1), (1, -4, 1), (1, 16, 0), (1, 16, 17),
                       (1, 16, -1)):
        assert lib.hdf_cc_quantiles_workspace_bytes(c, cap, nq) == -1
        assert lib.hdf_last_error().startswith(b"components: quantiles:"), lib.hdf_last_error()
    up = lambda b: (b + 255) // 256 * 256                        # noqa: E731
    for c, cap, nq in ((1, 1, 1), (2, 4096, 3), (3, 77, 16), (8, 65536, 16)):
        # n and the coordinate sums, then the boxes; every part on a 256-byte boundary
        assert lib.hdf_cc_quantiles_workspace_bytes(c, cap, nq) == up(cap * 32) + up(cap * 24)


def test_every_refusal_comes_before_a_launch(lib):
    """HDF_ERR_ARG = 1 with a "components: quantiles:" message.  No device address is dereferenced: on this host, which has
    no device, a memset or a launch would come back as HDF_ERR_HIP = 2."""
    Cn, D, H, W, cap, Q = 2, 3, 5, 7, 10, 3
    V = D * H * W
    need = lib.hdf_cc_quantiles_workspace_bytes(Cn, cap, Q)
    assert need > 0
    levels = (C.c_double * 16)(0.1, 0.5, 0.9)
    base = 0x10000000                                            # made-up, aligned, far apart
    good = dict(ids=base, image=base + 0x100000, C=Cn, D=D, H=H, W=W, cap=cap, q=levels, Q=Q, count=base + 0x200000,
                values=base + 0x300000, res=base + 0x500000, ws=base + 0x600000, ws_bytes=need)

    def call(**kw):
        a = dict(good, **kw)
        rc = lib.hdf_cc_quantiles(a["ids"], a["image"], a["C"], a["D"], a["H"], a["W"], a["cap"], a["q"], a["Q"], a["count"],
                                  a["values"], a["res"], a["ws"], a["ws_bytes"], None)
        return rc, lib.hdf_last_error().decode()

    def lv(*v):
        return (C.c_double * 16)(*v)

    bad = [dict(C=0), dict(C=9), dict(C=-1), dict(D=0), dict(H=1025), dict(W=-1), dict(D=1025), dict(cap=0), dict(cap=65537),
           dict(cap=-1), dict(ids=None), dict(image=None), dict(count=None), dict(values=None), dict(res=None), dict(ws=None),
           dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(ws=good["ws"] + 4, ws_bytes=need + 8),
           dict(count=good["count"] + 4), dict(values=good["values"] + 2), dict(res=good["res"] + 1),
           dict(Q=0), dict(Q=17), dict(Q=-3), dict(q=None), dict(q=lv(0.1, float("nan"), 0.9)), dict(q=lv(-1e-300, 0.5, 0.9)),
           dict(q=lv(0.1, 0.5, np.nextafter(1.0, 2.0))), dict(q=lv(0.1, float("inf"), 0.9)), dict(q=lv(0.5, -0.5), Q=2)]
    ids, img = good["ids"], good["image"]
    sizes = dict(count=cap * 8, values=Cn * cap * Q * 24, res=32, ws=need)
    for name, nbytes in sizes.items():
        bad += [{name: ids}, {name: ids + 4 * V - 8}, {name: ids - nbytes + 8}, {name: img + 8}, {name: img + 4 * Cn * V - 8},
                {name: img + 4 * V}]                              # the second channel is input too
        for other, obytes in sizes.items():
            if other != name:
                bad += [{name: good[other] + obytes - 8}, {name: good[other] - nbytes + 8}]
    for kw in bad:
        rc, msg = call(**kw)
        assert rc == 1 and msg.startswith("components: quantiles:"), (kw, rc, msg)
    # the levels at the ends of the range, -0 among them, are not refused for their value: the next check answers
    rc, msg = call(q=lv(0.0, 1.0, -0.0), ws_bytes=0)
    assert rc == 1 and "workspace" in msg, msg
