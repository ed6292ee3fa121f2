"""tests/measure_ref.py, the restatement the GPU test of hdf_cc_measure compares with, held to live scipy.ndimage
(sum_labels, mean, variance, minimum, maximum, center_of_mass, and minimum_position / maximum_position on tie-free inputs)
within its own derived bounds, to a plain per-component loop on inputs with ties, and to seven planted defects that its
comparison must name.  Then what can be checked of the entry without a GPU: every refusal comes before a launch, and the
Python layer exports the feature."""
import ctypes as C
import importlib.util
import math
import os

import numpy as np
import pytest
from scipy import ndimage as ndi

import measure_ref as mr
from conftest import ROOT

BIG = mr.BIG


def _as_got(want):
    return {k: np.array(want[k], copy=True) for k in ("geom", "stats", "pos", "result")}


def _tie_free(shape, C_):
    """every value once: a permutation of 0 .. V-1 (exact in float32), shifted to both signs"""
    V = int(np.prod(shape))
    assert V < 2 ** 24
    rng = np.random.default_rng(5)
    return np.stack([(rng.permutation(V) - V // 3).astype(np.float32).reshape(shape) for _ in range(C_)])


# ------------------------------------------------------------------------------------------------ against scipy
@pytest.mark.parametrize("kind", ["uniform", "constant", "levels", "signed", "tie_free"])
@pytest.mark.parametrize("ids_key", [("label", "rand20", 6), ("label", "full", 26), ("special", "classes"), ("special", "gaps")],
                         ids=lambda k: "-".join(map(str, k)))
def test_the_restatement_against_scipy(kind, ids_key):
    ids = mr.labelled(BIG, ids_key[1], ids_key[2])[0] if ids_key[0] == "label" else mr.special_ids(BIG, ids_key[1])[0]
    cap = int(ids.max())
    img = _tie_free(BIG, 1) if kind == "tie_free" else mr.image(kind, BIG, 1)
    want = mr.measure(ids, img, cap)
    lab = np.where(ids < 0, 0, ids)
    index = np.arange(1, cap + 1)
    x = img[0].astype(np.float64)
    n = np.asarray(ndi.sum_labels(np.ones(BIG), lab, index))
    assert np.array_equal(np.rint(n).astype(np.int64), want["geom"][:, 0])
    present = want["geom"][:, 0] > 0
    assert present.sum() >= (1 if ids_key[1] == "full" else 3)
    ip = index[present]
    nn = np.maximum(want["geom"][:, 0], 1).astype(np.float64)
    got = _as_got(want)
    got["stats"][0, present, 0] = ndi.sum_labels(x, lab, ip)
    got["stats"][0, present, 1] = ndi.mean(x, lab, ip)
    with np.errstate(invalid="ignore"):                          # (scipy forms the mean of every label up to the largest)
        got["stats"][0, present, 2] = np.asarray(ndi.variance(x, lab, ip)) * nn[present]
    got["stats"][0, present, 3] = np.asarray(ndi.minimum(x, lab, ip)) + 0.0
    got["stats"][0, present, 4] = np.asarray(ndi.maximum(x, lab, ip)) + 0.0
    print("scipy's sums, means and variances: worst error / bound = %.3g" % mr.worst(got, want))
    assert mr.mismatches(got, want) == []
    # geometric centroid (exact integers) and the weighted centre of mass, to the bounds of W and S1 carried through W / S1
    cen = np.asarray(ndi.center_of_mass(np.ones(BIG), lab, index[present]))
    assert np.allclose(cen, want["geom"][present, 1:] / nn[present, None], rtol=1e-13, atol=0)
    b = mr.bounds(want)[0]
    s1 = want["stats"][0, :, 0]
    ok = present & (b[:, 0] <= 2.0 ** -20 * np.abs(s1))           # (a component that sums to about 0 has no stable centre)
    # (uniform and constant are positive; four levels with a negative one can cancel; the two signed kinds do)
    assert ok.sum() >= {"uniform": 1.0, "constant": 1.0, "levels": 0.9}.get(kind, 0.0) * present.sum() and ok.any()
    com = np.asarray(ndi.center_of_mass(x, lab, index[ok]))
    for k in range(3):
        ref = want["stats"][0, ok, 5 + k] / s1[ok]
        tol = (b[ok, 5 + k] + np.abs(ref) * b[ok, 0]) / np.abs(s1[ok]) * (1 + 2.0 ** -19) + 3 * mr.U * np.abs(ref)
        assert (np.abs(com[:, k] - ref) <= tol).all(), (k, float(np.max(np.abs(com[:, k] - ref) / np.maximum(tol, 1e-300))))
    if kind == "tie_free":
        for col, fn in ((0, ndi.minimum_position), (1, ndi.maximum_position)):
            p = np.asarray(fn(x, lab, index[present]))
            assert np.array_equal(np.ravel_multi_index(tuple(p.T), BIG), want["pos"][0, present, col])


def test_the_centre_of_mass_of_a_component_that_sums_to_zero_is_scipys():
    ids = np.zeros((1, 2, 4), np.int32)
    ids[0, 0, :2], ids[0, 1, :2], ids[0, 1, 2:] = 1, 2, 3
    img = np.zeros((1, 1, 2, 4), np.float32)
    img[0, 0, 0, :2] = (1.0, -1.0)                               # sums to 0 with W != 0: an infinity; all zeros: nan
    img[0, 0, 1, 2:] = (2.0, 4.0)
    d = mr.dicts(mr.measure(ids, img, 3), (1, 2, 4))
    with np.errstate(divide="ignore", invalid="ignore"):
        sci = ndi.center_of_mass(img[0].astype(np.float64), ids, [1, 2, 3])
    for got, want in zip(d, sci):
        for a, b in zip(got["channels"][0]["center_of_mass"], want):
            assert (math.isnan(a) and math.isnan(b)) or a == b, (got, want)
    assert d[0]["channels"][0]["center_of_mass"][2] == -math.inf and math.isnan(d[1]["channels"][0]["center_of_mass"][0])


# ------------------------------------------------------------------------------------------------ ties: a plain loop
@pytest.mark.parametrize("kind", ["levels", "constant", "zeros_denormals", "ints"])
def test_the_restatement_against_a_plain_loop_on_ties(kind):
    shape = (5, 17, 33)
    ids = mr.special_ids(shape, "classes")[0]
    img = mr.image(kind, shape, 2)
    want = mr.measure(ids, img, 5)
    zz, yy, xx = np.indices(shape)
    for c in range(2):
        for i in range(1, 6):
            m = ids == i
            r = want["stats"][c, i - 1]
            if not m.any():
                assert not want["geom"][i - 1].any() and not r.any() and not want["pos"][c, i - 1].any()
                continue
            v = img[c][m].astype(np.float64)
            where = np.flatnonzero(m.ravel())
            assert want["geom"][i - 1].tolist() == [int(m.sum()), int(zz[m].sum()), int(yy[m].sum()), int(xx[m].sum())]
            assert r[3] == v.min() and r[4] == v.max()
            first_min = next(int(w) for w, val in zip(where, v) if val == v.min())
            first_max = next(int(w) for w, val in zip(where, v) if val == v.max())
            assert want["pos"][c, i - 1].tolist() == [first_min, first_max]
            assert r[0] == math.fsum(v) and r[1] == r[0] / m.sum() and r[5] == math.fsum(zz[m] * v)
            assert r[2] == math.fsum((v - r[1]) ** 2) and r[6] == math.fsum(yy[m] * v) and r[7] == math.fsum(xx[m] * v)
    if kind == "zeros_denormals":
        ext = want["stats"][..., 3:5]
        assert (img.view(np.uint32) == 0x80000000).any() and (ext == 0).any() and not np.signbit(ext[ext == 0]).any()


# ------------------------------------------------------------------------------------------------ planted defects
def _defect_case():
    """one full-volume component, a class map and four-level / signed images: every defect below shows on one of them"""
    shape = (6, 11, 23)
    return shape, mr.special_ids(shape, "classes")[0], np.ones(shape, np.int32)


def _group(ids, img_c, i):
    where = np.flatnonzero(ids.ravel() == i)
    return where, img_c.ravel()[where].astype(np.float64)


def test_planted_defects_are_named():
    shape, classes, full = _defect_case()
    levels, signed = mr.image("levels", shape, 1), mr.image("signed", shape, 1)
    zz, yy, xx = (a.astype(np.float64) for a in np.indices(shape))

    # 1. the LAST index on a tie (scipy's maximum_position): four levels, so every extremum is tied
    want = mr.measure(classes, levels, 3)
    got = _as_got(want)
    for i in (1, 2, 3):
        where, v = _group(classes, levels[0], i)
        got["pos"][0, i - 1] = where[np.flatnonzero(v == v.min())[-1]], where[np.flatnonzero(v == v.max())[-1]]
    assert mr.mismatches(got, want) == ["argmin", "argmax"]

    # 2. n - 1 in the variance: an M2 that turns into the sample variance when divided by n
    got = _as_got(want)
    n = want["geom"][:, 0].astype(np.float64)
    got["stats"][0, :, 2] *= n / (n - 1)
    assert mr.mismatches(got, want) == ["m2"]

    # 3. an unweighted centre of mass: W = (sum z) * mean
    got = _as_got(want)
    for k in range(3):
        got["stats"][0, :, 5 + k] = want["geom"][:, 1 + k] * want["stats"][0, :, 1]
    assert mr.mismatches(got, want) == ["wz", "wy", "wx"]

    # 4. y and x swapped
    got = _as_got(want)
    got["geom"][:, [2, 3]] = want["geom"][:, [3, 2]]
    got["stats"][0][:, [6, 7]] = want["stats"][0][:, [7, 6]]
    assert mr.mismatches(got, want) == ["sum_y", "sum_x", "wy", "wx"]

    # 5. negative values ordered by their raw bits with the sign flipped only: among negatives the order is reversed
    want = mr.measure(classes, signed, 3)
    got = _as_got(want)
    for i in (1, 2, 3):
        where, v = _group(classes, signed[0], i)
        key = signed[0].ravel()[where].view(np.uint32) ^ np.uint32(0x80000000)
        lo = int(np.argmin(key))
        got["stats"][0, i - 1, 3], got["pos"][0, i - 1, 0] = v[lo], where[lo]
    assert mr.mismatches(got, want) == ["argmin", "min"]

    # 6. ids above the capacity folded into the last row
    want = mr.measure(classes, levels, 2)
    folded = mr.measure(np.minimum(classes, 2), levels, 2)
    bad = mr.mismatches(_as_got(folded), want)
    assert "n" in bad and "sum" in bad and "result" in bad

    # 7. a voxel on a slab boundary counted twice in the fp64 sums of the full-volume component
    want = mr.measure(full, signed, 1)
    got = _as_got(want)
    v = int(np.prod(shape)) // 8
    x = float(signed[0].ravel()[v])
    got["stats"][0, 0, 0] += x
    got["stats"][0, 0, 5:] += np.array([zz.ravel()[v], yy.ravel()[v], xx.ravel()[v]]) * x
    bad = mr.mismatches(got, want)
    assert "sum" in bad and "wx" in bad and "n" not in bad
    # ... and in M2 alone
    got = _as_got(want)
    got["stats"][0, 0, 2] += (x - want["stats"][0, 0, 1]) ** 2
    assert mr.mismatches(got, want) == ["m2"]

    # nothing planted: nothing named; one ulp in a sum of small integers is named (the bound is n u sum|t|, not a tolerance)
    assert mr.mismatches(_as_got(want), want) == []
    one = mr.measure(classes[:1, :1, :2] * 0 + 1, np.float32([[[[3.0, 5.0]]]]), 1)
    got = _as_got(one)
    got["stats"][0, 0, 0] = np.nextafter(8.0, 9.0)
    assert mr.mismatches(got, one) == [] and 2 * mr.U * 8.0 >= np.nextafter(8.0, 9.0) - 8.0        # inside n u sum|t|: two terms
    got["stats"][0, 0, 0] = 8.0 + 4 * (np.nextafter(8.0, 9.0) - 8.0)
    assert mr.mismatches(got, one) == ["sum"]
    zero = mr.measure(classes[:1, :1, :2] * 0 + 1, np.float32([[[[-0.0, 5.0]]]]), 1)
    assert zero["stats"][0, 0, 3] == 0.0 and not np.signbit(zero["stats"][0, 0, 3])
    got = _as_got(zero)
    got["stats"][0, 0, 3] = -0.0
    assert mr.mismatches(got, zero) == ["min"]                   # min and max are compared as bits: a -0 is not the +0 asked for


def test_absent_rows_must_be_zero_bytes():
    ids, top = mr.special_ids((4, 10, 25), "gaps")
    want = mr.measure(ids, mr.image("uniform", (4, 10, 25), 2), top + 3)
    assert (want["geom"][:, 0] == 0).sum() >= 30
    got = _as_got(want)
    got["pos"][1, 0, 1] = 7                                      # id 1 is absent
    assert mr.mismatches(got, want) == ["argmax", "absent rows"]
    got = _as_got(want)
    got["stats"][0, 1, 2] = -0.0
    assert mr.mismatches(got, want) == ["absent rows"]


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
    assert callable(hdf_rt.region_stats) and callable(hdf_rt.region_measure) and callable(hdf_rt.pet_lesion_measures)
    assert "hdf_cc_measure" in _lib.EXPORTS and "hdf_cc_measure_workspace_bytes" in _lib.EXPORTS
    assert {"region_measure", "region_stats", "pet_lesion_measures"} <= set(dir(hdf_rt))


def test_the_workspace_size(lib):
    for c, cap in ((0, 16), (9, 16), (-1, 16), (1, 0), (1, 65537), (1, -4)):
        assert lib.hdf_cc_measure_workspace_bytes(c, cap) == -1
        assert lib.hdf_last_error().startswith(b"components: measure:"), lib.hdf_last_error()
    up = lambda b: (b + 255) // 256 * 256                        # noqa: E731
    for c, cap in ((1, 1), (2, 4096), (3, 77), (8, 65536)):
        # the boxes, the two keys a channel, eight slabs of four fp64 a channel; every part on a 256-byte boundary
        assert lib.hdf_cc_measure_workspace_bytes(c, cap) == up(cap * 24) + up(c * cap * 16) + up(c * cap * 8 * 4 * 8)


def test_every_refusal_comes_before_a_launch(lib):
    """HDF_ERR_ARG = 1 with a "components: measure:" message.  No address is dereferenced: on this host, which has no
    device, a memset or a launch would come back as HDF_ERR_HIP = 2."""
    Cn, D, H, W, cap = 2, 3, 5, 7, 10
    V = D * H * W
    need = lib.hdf_cc_measure_workspace_bytes(Cn, cap)
    assert need > 0
    base = 0x10000000                                            # made-up, aligned, far apart
    good = dict(ids=base, image=base + 0x100000, C=Cn, D=D, H=H, W=W, cap=cap, geom=base + 0x200000, stats=base + 0x300000,
                pos=base + 0x400000, res=base + 0x500000, ws=base + 0x600000, ws_bytes=need)

    def call(**kw):
        a = dict(good, **kw)
        rc = lib.hdf_cc_measure(a["ids"], a["image"], a["C"], a["D"], a["H"], a["W"], a["cap"], a["geom"], a["stats"], a["pos"],
                                a["res"], a["ws"], a["ws_bytes"], None)
        return rc, lib.hdf_last_error().decode()

    bad = [dict(C=0), dict(C=9), dict(C=-1), dict(D=0), dict(H=1025), dict(W=-1), dict(D=1025), dict(cap=0), dict(cap=65537),
           dict(cap=-1), dict(ids=None), dict(image=None), dict(geom=None), dict(stats=None), dict(pos=None), dict(res=None),
           dict(ws=None), dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(ws=good["ws"] + 4, ws_bytes=need + 8),
           dict(geom=good["geom"] + 4), dict(stats=good["stats"] + 4), dict(pos=good["pos"] + 2), dict(res=good["res"] + 1)]
    # an output or the workspace over an input, over another output, over the workspace: first byte, last byte, inside
    ids, img = good["ids"], good["image"]
    sizes = dict(geom=cap * 32, stats=Cn * cap * 64, pos=Cn * cap * 16, res=32, ws=need)
    for name, nbytes in sizes.items():
        bad += [{name: ids}, {name: ids + 4 * V - 8}, {name: ids - nbytes + 8}, {name: img + 8}, {name: img + 4 * Cn * V - 8},
                {name: img + 4 * V}]                              # the second channel is input too
        for other, obytes in sizes.items():
            if other != name:
                bad += [{name: good[other] + obytes - 8}, {name: good[other] - nbytes + 8}]
    for kw in bad:
        rc, msg = call(**kw)
        assert rc == 1 and msg.startswith("components: measure:"), (kw, rc, msg)
