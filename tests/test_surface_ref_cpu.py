"""Host-side checks of the surface-distance path (no GPU):
  * tests/surface_ref.py, the scipy restatement the GPU tests compare against, held to independent definitions -- an
    all-pairs brute force for the distance map and both border sets, np.percentile of the fp64 square roots for the
    percentile (1e-12 relative) -- on volumes of about 5x6x7;
  * four planted defects (a 6-connected border, the volume edge as background, a nearest-rank percentile, HD over the
    contours only): each must change a quantity that tests/test_gpu_surface.py compares (flags, a distance map, the
    histogram, the result integers) on that test's own inputs, so those inputs can see it;
  * the C ABI's refusals, which happen before anything is launched, and the wrappers' HdfError without a device."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest
import torch

import surface_ref as sr
from conftest import ROOT


# ---------------------------------------------------------------------------------- the restatement against brute force
def _brute_border(mask, offsets):
    out = np.zeros_like(mask)
    for v in zip(*np.nonzero(mask)):
        for o in offsets:
            n = tuple(a + b for a, b in zip(v, o))
            if all(0 <= c < s for c, s in zip(n, mask.shape)) and not mask[n]:
                out[v] = True
    return out


OFF26 = [o for o in itertools.product((-1, 0, 1), repeat=3) if any(o)]
OFF6 = [o for o in OFF26 if sum(map(abs, o)) == 1]


def _brute_d2(seed):
    pts = np.argwhere(seed)
    if len(pts) == 0:
        return np.full(seed.shape, sr.NO_SEED, np.int64)
    grid = np.indices(seed.shape).reshape(3, -1).T
    return ((grid[:, None, :] - pts[None, :, :]) ** 2).sum(-1).min(1).reshape(seed.shape)


@pytest.mark.parametrize("shape,seed", [((5, 6, 7), 0), ((5, 6, 7), 1), ((6, 5, 7), 2), ((1, 6, 7), 3), ((7, 1, 5), 4)])
def test_restatement_equals_brute_force(shape, seed):
    t, p = sr.blobs(shape, seed, 0.3)
    ref = sr.surface(t, p, 1)
    T, P = t == 1, p == 1
    assert 0 < T.sum() < T.size and 0 < P.sum() < P.size
    bT, bP = _brute_border(T, OFF26), _brute_border(P, OFF26)
    cT, cP = _brute_border(T, OFF6), _brute_border(P, OFF6)
    want = T * 1 + P * 2 + bT * 4 + bP * 8 + cT * 16 + cP * 32
    assert np.array_equal(ref["flags"], want)
    assert np.array_equal(ref["d2T"], _brute_d2(bT)) and np.array_equal(ref["d2P"], _brute_d2(bP))
    S = np.sort(np.concatenate([_brute_d2(bT)[cP], _brute_d2(bP)[cT]]))
    assert np.array_equal(np.repeat(np.arange(len(ref["hist"])), ref["hist"]), S)
    res = ref["result"]
    assert res[:5] == [T.sum(), P.sum(), (T & P).sum(), cT.sum(), cP.sum()] and res[6] == len(S) and res[11] == 1
    assert res[5] == max(_brute_d2(bT)[P & ~T].max(initial=0), _brute_d2(bP)[T & ~P].max(initial=0))
    got = sr.scores(res)
    want95 = np.percentile(np.sqrt(S.astype(np.float64)), 95)
    assert abs(got["HausdorffDistance95"] - want95) <= 1e-12 * want95
    assert got["Dice"] == 2 * (T & P).sum() / (T.sum() + P.sum())


@pytest.mark.parametrize("n", [1, 2, 3, 19, 20, 21, 22, 100, 101, 12345])
def test_integer_percentile_equals_numpy_linear(n):
    rng = np.random.default_rng(n)
    S = np.sort(rng.integers(0, 400, n))
    lo, r, hi = sr.select(n)
    a, b = np.sqrt(float(S[lo])), np.sqrt(float(S[hi]))
    want = np.percentile(np.sqrt(S.astype(np.float64)), 95)
    assert abs(a + (b - a) * r / 100 - want) <= 1e-12 * max(want, 1e-300)


def test_no_seed_and_degenerate_masks():
    z = np.zeros((3, 4, 5), np.uint8)
    assert (sr.d2_of(z.astype(bool)) == sr.NO_SEED).all()
    p = z.copy()
    p[1, 1, 1] = 1
    for t, q in ((z, p), (p, z), (z, z), (z + 1, p), (p, z + 1)):
        res = sr.surface(t, q, 1)["result"]
        assert res[5:] == [0] * 7
        s = sr.scores(res)
        assert np.isnan(s["HausdorffDistance"]) and np.isnan(s["HausdorffDistance95"])
    s = sr.scores(sr.surface(z, z, 1)["result"])
    assert all(np.isnan(s[k]) for k in ("Dice", "Jaccard", "VolumeSimilarity"))
    assert sr.scores(sr.surface(z, p, 1)["result"])["VolumeSimilarity"] == -2.0     # 2 (nT - nP) / (nT + nP)


# -------------------------------------------------------------------------------------------------- planted defects
def _differs(a, b):
    return (not np.array_equal(a["flags"], b["flags"]) or not np.array_equal(a["d2T"], b["d2T"])
            or not np.array_equal(a["d2P"], b["d2P"]) or not np.array_equal(a["hist"], b["hist"])
            or a["result"] != b["result"])


@pytest.mark.parametrize("defect", sr.DEFECTS)
def test_gpu_inputs_can_see_each_planted_defect(defect):
    seen = []
    for shape in sr.SHAPES:
        for kind in ("blobs", "faces", "distant"):
            t, p, k = sr.case(shape, kind)
            if _differs(sr.case_ref(shape, kind), sr.surface(t, p, k, defect=defect)):
                seen.append((shape, kind))
    assert len(seen) >= 2, seen


def test_gpu_inputs_are_what_their_names_say():
    for shape in sr.SHAPES[1:]:
        t, p, k = sr.case(shape, "faces")
        T = t == k
        assert T[0].any() or T[-1].any() or T[:, 0].any() or T[:, -1].any() or T[..., 0].any() or T[..., -1].any()
        assert sr.case_ref(shape, "faces")["result"][11] == 1 and sr.case_ref(shape, "blobs")["result"][11] == 1
        res = sr.case_ref(shape, "corners")["result"]
        assert res[11] == 1 and res[5] == sum((s - 1) ** 2 for s in shape) and res[2] == 0
        res = sr.case_ref(shape, "identical")["result"]
        assert res[11] == 1 and res[5] == 0 and res[7] == 0 and res[8] == 0 and res[0] == res[2]
        assert sr.case_ref(shape, "distant")["result"][2] == 0 and sr.case_ref(shape, "distant")["result"][11] == 1
        for kind in ("empty_t", "empty_p", "empty_both", "full"):
            assert sr.case_ref(shape, kind)["result"][11] == 0
    assert sr.case_ref((1024, 2, 3), "corners")["result"][5] == 1046534
    tl, pl = sr.label_maps((40, 48, 56), 3, 3)
    assert all((tl == k).any() and (pl == k).any() for k in (1, 2, 3))


# -------------------------------------------------------------------------------------------------- the C ABI on the host
@pytest.fixture(scope="module")
def lib():
    from hdf_rt import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import importlib.util
        spec = importlib.util.spec_from_file_location("hdf_build", os.path.join(ROOT, "h-denseformer_amd", "build.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mod.build(verbose=False)
    return _lib.lib()


def test_surface_entries_refuse_bad_arguments_before_any_launch(lib):
    """HDF_ERR_ARG (1) with a "surface:" message; on this host, which has no device, a memset or a launch would come back
    as HDF_ERR_HIP (2).  The addresses are never dereferenced."""
    buf = (C.c_uint64 * 16)()
    a = C.addressof(buf)
    big = 1 << 40

    def all_three(D, H, W, label, ws_bytes):
        return [lib.hdf_op_mask_flags(a, a, label, D, H, W, a, a, None),
                lib.hdf_op_edt_sq(a, 4 if label else 0, D, H, W, a, a, ws_bytes, None),
                lib.hdf_surface_distances(a, a, label, D, H, W, a, ws_bytes, a, None, 0, None)]

    # (with every dimension capped at 1024 a product of 2^31 needs a dimension past the cap: refused either way)
    bad_dims = [(0, 8, 8), (8, 0, 8), (8, 8, 0), (1025, 8, 8), (8, 1025, 8), (8, 8, 1025), (-3, 8, 8),
                (2048, 1024, 1024), (1024, 1024, 2048), (65536, 65536, 1)]
    for dims in bad_dims:
        assert lib.hdf_surface_workspace_bytes(*dims) == -1 and lib.hdf_last_error().startswith(b"surface:")
        for rc in all_three(*dims, 1, big):
            assert rc == 1 and lib.hdf_last_error().startswith(b"surface:"), (dims, rc, lib.hdf_last_error())
    for label in (0, 256, -1):
        rcs = all_three(8, 8, 8, label, big)
        assert rcs[0] == 1 and rcs[2] == 1 and lib.hdf_last_error().startswith(b"surface:"), (label, rcs)
    assert lib.hdf_op_edt_sq(a, 0, 8, 8, 8, a, a, big, None) == 1 and lib.hdf_last_error().startswith(b"surface:")
    need = lib.hdf_surface_workspace_bytes(8, 9, 10)
    assert need > 0
    for short in (0, need - 1):
        assert lib.hdf_op_edt_sq(a, 4, 8, 9, 10, a, a, short, None) == 1 and lib.hdf_last_error().startswith(b"surface:")
        assert lib.hdf_surface_distances(a, a, 1, 8, 9, 10, a, short, a, None, 0, None) == 1
        assert lib.hdf_last_error().startswith(b"surface:")
    assert lib.hdf_surface_distances(a, a, 1, 8, 9, 10, a, need, a, None, -1, None) == 1


def test_workspace_size_is_positive_and_monotone(lib):
    f = lib.hdf_surface_workspace_bytes
    assert f(1, 1, 1) > 0
    prev = 0
    for n in (1, 2, 3, 17, 64, 144, 240, 1024):
        assert f(n, n, 1) >= prev          # (parts are rounded up to 256 bytes: small volumes tie)
        prev = f(n, n, 1)
        for a, b in (((n, 5, 7), (n + 1 if n < 1024 else n, 5, 7)), ((5, n, 7), (5, n, 8)), ((5, 7, n), (6, 7, n))):
            assert f(*b) >= f(*a) > 0
    # flags + two int32 maps + the histogram: at least 9 bytes a voxel; the largest volume is accepted
    assert f(240, 240, 155) >= 9 * 240 * 240 * 155 and f(144, 144, 144) > f(64, 64, 64) > f(8, 8, 8)
    assert f(1024, 1024, 1024) >= 9 * 2 ** 30


def test_wrappers_fail_loudly_without_a_device(monkeypatch):
    from hdf_rt import HdfError, cal_score, multi_dice, multi_hd, multi_jc, multi_vs
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)     # (so that the test is the same where there is one)
    t, p = sr.label_maps((8, 9, 10), 1, 2)
    for fn in (multi_hd, multi_dice, multi_vs, multi_jc):
        with pytest.raises(HdfError):
            fn(t, p, 2)
    with pytest.raises(HdfError):
        cal_score(p == 1, t == 1)
    with pytest.raises(HdfError):
        multi_hd(torch.from_numpy(t), torch.from_numpy(p), 2)
