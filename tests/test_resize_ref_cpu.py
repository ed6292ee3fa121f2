"""tests/resize_ref.py, the fp64 restatement that the GPU tests of hdf_resize_3d compare against, held to live scipy (the
arithmetic of skimage.transform.resize(order=1); scikit-image itself is not a dependency), plus what runs without a
device: TrainTransform3D.from_ids and the entries' refusals.

  (a) every listed shape x both boundary modes x C in {1, 2}: restatement == scipy within (g + 1) 2^-24 vmax per element
      (scipy's own fp32 roundings; seen: at most 0.83 of ONE such unit)
        9x37x43 -> 6x24x48       down, down, up            5x20x22 -> 7x31x29    all up, no filter
        8x37x43 -> 1x24x48       f = 8, r = 14 > n_in: the reflection repeats     1x37x43 -> 1x24x48    an n = 1 axis
        16x3x8 -> 2x3x1          f = 8 on two axes         7x40x48 -> 7x20x24    identity axis + exact factor 2
        104x101x103 -> 53x80x111 the GPU tests' volume past the grid caps
  (b) class maps equal scipy's outside the 1e-7 band around 0.5; the band is EMPTY for the blocky labels on every shape
      (the condition the GPU tests rely on) and <= 1e-4 for the noisy ones, except 5x20x22 -> 7x31x29 (50 genuine ties)
  (c) five planted defects are caught
  (d) from_ids: settings, refusals, draws
  (e) the entries are exported, refuse bad arguments without a device and have no CPU path"""
import ctypes as C
import functools
import os
import random

import numpy as np
import pytest
import torch

import augment_ref as ar
import resize_ref as rr
from conftest import ROOT

MODES = ("mirror", "constant")
IDS = ["%dx%dx%d-%dx%dx%d" % (a + b) for a, b in rr.SHAPES]


@functools.lru_cache(maxsize=None)
def _image(shape):
    img = ar.image_of(shape, 2, 1)
    img.setflags(write=False)
    return img


# ------------------------------------------------------------------------------------------------- (a) against scipy
@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("src,dst", rr.SHAPES, ids=IDS)
def test_restatement_equals_scipy_to_its_own_roundings(src, dst, mode, channels):
    worst = 0.0
    for ch in _image(src)[:channels] if channels == 2 else _image(src)[1:]:     # C = 1: the channel scaled by 1e4
        ref, g = rr.resize_plane(ch, dst, mode)
        worst = max(worst, rr.check_against_scipy(ref, rr.scipy_plane(ch, dst, mode), g, np.abs(ch).max(),
                                                  "%s %s" % (mode, src)))
    print("RESIZE-REF %s -> %s %s C%d: worst %.3f units of 2^-24 vmax, bound %d" % (src, dst, mode, channels, worst, g + 1))
    assert worst <= g + 1


def test_filtered_axes_and_radii_are_the_ones_the_cases_claim():
    assert [sum(rr.sigma_of(i, o) > 1e-15 for i, o in zip(a, b)) for a, b in rr.SHAPES] == [2, 0, 2, 1, 2, 2, 2]
    assert int(4 * rr.sigma_of(8, 1) + 0.5) == 14 and 14 > 8                     # the reflection repeats
    assert int(4 * rr.sigma_of(37, 24) + 0.5) == 1 and int(4 * rr.sigma_of(37, 24)) == 1
    assert int(4 * rr.sigma_of(9, 6) + 0.5) == 1 and int(4 * rr.sigma_of(40, 20) + 0.5) == 2


# ---------------------------------------------------------------------------------------------------- (b) class maps
@pytest.mark.parametrize("src,dst", rr.SHAPES, ids=IDS)
def test_class_maps_equal_scipy_outside_the_band_and_blocky_labels_have_none(src, dst):
    for blocky in (True, False):
        labels = ar.labels_of(src, 4, 1, blocky=blocky)
        assert (labels == 200).any() and (labels == 255).any()
        ref = rr.resize_ref(None, labels, 4, dst)
        _, sums32, got = rr.scipy_pipeline(None, labels, 4, dst)
        share = rr.check_maps_outside_band(ref["labels"], got, ref["sums"], "blocky" if blocky else "noisy")
        rr.check_against_scipy(ref["sums"], sums32, ref["g"], 1.0, "class sums")
        print("RESIZE-REF %s -> %s %s labels: band %.2e" % (src, dst, "blocky" if blocky else "noisy", share))
        if blocky:
            assert share == 0.0                    # what tests/test_gpu_resize.py relies on: nothing to exclude
            ar.check_labels(ref["labels"], ref["sums"])
        elif (src, dst) != rr.SHAPES[1]:
            assert share <= 1e-4
        else:
            assert share > 1e-4                    # 50 genuine ties: this shape is used with blocky labels only


# ------------------------------------------------------------------------------------------------ (c) planted defects
def _defect_is_caught(src, dst, mode, **defect):
    ch = _image(src)[0]
    good, g = rr.resize_plane(ch, dst, mode)
    want = rr.scipy_plane(ch, dst, mode)
    rr.check_against_scipy(good, want, g, np.abs(ch).max())
    bad, _ = rr.resize_plane(ch, dst, mode, **defect)
    with pytest.raises(AssertionError, match="outside the bound"):
        rr.check_against_scipy(bad, want, g, np.abs(ch).max())


def test_reflect_in_place_of_mirror_is_caught():
    _defect_is_caught(rr.SHAPES[0][0], rr.SHAPES[0][1], "mirror", reflect=True)
    _defect_is_caught(rr.SHAPES[1][0], rr.SHAPES[1][1], "mirror", reflect=True)      # in the interpolation alone


def test_truncated_radius_is_caught():
    # the listed shapes round 4 sigma alike either way (8 -> 1: 14.0; 40 -> 20: 2.0; 37 -> 24: 1.08), so take a factor
    # where it has a fraction of one half: 9 -> 4, sigma 0.625, 4 sigma = 2.5, radius 3 against 2
    assert int(4 * rr.sigma_of(9, 4) + 0.5) == 3 and int(4 * rr.sigma_of(9, 4)) == 2
    _defect_is_caught((9, 18, 27), (4, 8, 12), "mirror", radius_floor=True)
    _defect_is_caught((9, 18, 27), (4, 8, 12), "constant", radius_floor=True)


def test_dropped_half_is_caught():
    for mode in MODES:
        _defect_is_caught(rr.SHAPES[0][0], rr.SHAPES[0][1], mode, no_half=True)


def _tie_labels():
    """2:3 along W without a filter: output 1 reads c = 0.5 and output 4 c = 2.5, exactly between two voxels"""
    labels = np.zeros((2, 3, 4), dtype=np.uint8)
    labels[..., :] = [1, 2, 1, 0]
    return labels, (2, 3, 6)


def test_exclusive_threshold_is_caught_on_an_exact_half():
    labels, dst = _tie_labels()
    ref = rr.resize_ref(None, labels, 3, dst)
    assert (ref["sums"][0, ..., 1] == 0.5).all() and (ref["sums"][1, ..., 1] == 0.5).all()      # exact, both classes
    assert (ref["sums"][0, ..., 4] == 0.5).all() and (ref["sums"][1, ..., 4] == 0.0).all()      # class 1 against 0
    _, _, got = rr.scipy_pipeline(None, labels, 3, dst)
    ar.check_exact(ref["labels"], got, "tie labels")                                            # no exclusion
    assert (got[..., 4] == 1).all()                                                 # a class beats background at 0.5
    with pytest.raises(AssertionError):
        ar.check_exact(rr.labels_from_sums(ref["sums"], inclusive=False), got)


def test_first_class_winning_is_caught():
    labels, dst = _tie_labels()
    ref = rr.resize_ref(None, labels, 3, dst)
    _, _, got = rr.scipy_pipeline(None, labels, 3, dst)
    assert (got[..., 1] == 2).all()                                                             # the last class wins
    with pytest.raises(AssertionError):
        ar.check_exact(rr.labels_from_sums(ref["sums"], last_wins=False), got)


# ------------------------------------------------------------------------------------------------------- (d) from_ids
def _settings(t):
    return (t.patch_size, t.normalize, t.resize, t.crop, t.mode, t.flip, t.scale, t.trunc_after)


def test_from_ids_maps_the_reference_lists():
    from hdf_rt import TrainTransform3D as T
    kw = dict(input_shape=(16, 32, 48), patch_size=(16, 40, 50), crop=2, scale=(-100, 200))
    want = {
        (2, 3, 4, 5, 6): ((None, "petct", (16, 32, 48), 2, "tr", "hv", None, False),
                          (None, "petct", (16, 32, 48), 2, "", "", None, False)),
        (1, 2, 4, 5, 6): (((16, 40, 50), "petct", None, 0, "tr", "hv", None, False),
                          ((16, 40, 50), "petct", None, 0, "", "", None, False)),
        (1, 8, 4, 5, 6): (((16, 40, 50), "mr", None, 0, "tr", "hv", None, False),
                          ((16, 40, 50), None, None, 0, "", "", None, False)),          # validation drops 8
        (1, 7, 4, 5, 6): (((16, 40, 50), "trunc", None, 0, "tr", "hv", (-100, 200), False),
                          ((16, 40, 50), None, None, 0, "", "", None, False)),          # ... and 7
        (2, 3, 4, 5, 6, 7): ((None, "petct", (16, 32, 48), 2, "tr", "hv", (-100, 200), True),
                             (None, "petct", (16, 32, 48), 2, "", "", None, False)),
    }
    for ids, (train, val) in want.items():
        assert _settings(T.from_ids(3, list(ids), **kw)) == train, ids
        assert _settings(T.from_ids(3, list(ids), train=False, **kw)) == val, ids
    t = T.from_ids(3, [7, 6, 7], scale=(0, 1))
    assert t.normalize == "trunc" and t.trunc_after and t.mode == "" and t.flip == ""
    # the constructor keeps its signature and defaults
    d = T(3)
    assert _settings(d) == (None, None, None, 0, "tr", "hv", None, False)
    assert _settings(T(3, (1, 2, 3), "mr", "t", "h")) == ((1, 2, 3), "mr", None, 0, "t", "h", None, False)


def test_from_ids_refuses_bad_orders_by_name():
    from hdf_rt import TrainTransform3D as T
    kw = dict(input_shape=(16, 32, 48), patch_size=(16, 40, 50), scale=(-100, 200))
    for bad in ([3, 2, 4, 5, 6], [2, 1, 6], [2, 8, 6], [4, 3, 6], [5, 4, 6], [6, 4], [2, 2, 6], [6, 7, 7], [6, 3]):
        with pytest.raises(ValueError, match="subsequence of 1, one of 2"):
            T.from_ids(3, bad, **kw)
    for missing in ([2, 3, 4, 5], [1, 7], []):
        with pytest.raises(ValueError, match=r"must hold 6 \(To_Tensor\)"):
            T.from_ids(3, missing, **kw)
    for unknown in ([0, 6], [9, 6]):
        with pytest.raises(ValueError, match="not in the reference's list"):
            T.from_ids(3, unknown, **kw)
    with pytest.raises(ValueError, match="needs input_shape"):
        T.from_ids(3, [2, 3, 6])
    with pytest.raises(ValueError, match="needs patch_size"):
        T.from_ids(3, [1, 6])
    with pytest.raises(ValueError, match="needs scale"):
        T.from_ids(3, [7, 6])
    with pytest.raises(ValueError, match="normalize must be"):
        T(3, normalize="ct")


def test_draws_follow_the_reference_order():
    from hdf_rt import TrainTransform3D as T, crop_origin, flip_flags, trz_matrix
    shape, patch = (20, 45, 50), (16, 40, 50)
    for ids in ([1, 2, 4, 5, 6], [2, 3, 4, 5, 6], [1, 2, 6], [2, 3, 5, 6]):
        t = T.from_ids(3, ids, input_shape=(16, 32, 48), patch_size=patch)
        for seed in (0, 7):
            random.seed(seed), np.random.seed(seed)
            origin, affine, flips = t.draw(shape)
            after = (random.getstate(), np.random.get_state()[1].copy(), np.random.get_state()[2])
            random.seed(seed), np.random.seed(seed)
            want_o = crop_origin(shape, patch) if 1 in ids else None
            want_a = trz_matrix("tr" if 4 in ids else "")
            want_f = flip_flags("hv" if 5 in ids else "")
            assert origin == want_o and np.array_equal(affine, want_a) and flips == want_f, ids
            assert random.getstate() == after[0] and np.array_equal(np.random.get_state()[1], after[1])
            assert np.random.get_state()[2] == after[2]                   # the resize drew nothing, nor anything else


# ---------------------------------------------------------------------------------------------------- (e) the entries
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


def test_entries_are_exported_as_declared(lib):
    import hdf_rt
    from hdf_rt import _lib
    hdr = open(os.path.join(ROOT, "include", "hdf.h")).read()
    for name in ("hdf_resize_workspace_bytes", "hdf_resize_3d", "hdf_trunc_normalize"):
        assert name in _lib.EXPORTS and hasattr(lib, name) and name + "(" in hdr, name
    assert len(_lib._PROTOS["hdf_resize_3d"][1]) == 15 and len(_lib._PROTOS["hdf_trunc_normalize"][1]) == 5
    for name in ("resize_3d", "crop_resize", "trunc_normalize_", "TrainTransform3D"):
        assert callable(getattr(hdf_rt, name)) and name in dir(hdf_rt), name
    assert callable(hdf_rt.TrainTransform3D.from_ids)


def test_workspace_holds_the_intermediates_of_one_plane(lib):
    ws = lib.hdf_resize_workspace_bytes
    assert ws(9, 37, 43, 9, 37, 43) == 0 and ws(9, 37, 43, 9, 24, 43) == 0            # at most one axis changes
    # 9x37x43 -> 6x24x48: H first (24/37), then D (6/9), W last (48/43 grows): 9x24x43 and 6x24x43 doubles
    assert ws(9, 37, 43, 6, 24, 48) == 8 * (9 * 24 * 43 + 6 * 24 * 43)
    # all three grow: the smallest growth first, the largest last
    assert ws(5, 20, 22, 7, 31, 29) == 8 * (5 * 20 * 29 + 7 * 20 * 29)
    # the datasets of config.py:69-74: never more than the source's size in doubles, whatever the channel count
    # (H and W shrink most and alike: the outer of the two first, D last)
    assert ws(448, 512, 512, 144, 144, 144) == 8 * (448 * 144 * 512 + 448 * 144 * 144)
    assert ws(1025, 8, 8, 8, 8, 8) == -1 and ws(65, 8, 8, 8, 8, 8) == -1 and ws(0, 8, 8, 8, 8, 8) == -1


def test_bad_arguments_are_refused_without_a_device(lib):
    buf = (C.c_double * 4096)()
    a = C.addressof(buf)
    img, lab, io, lo, ws = a, a + 8192, a + 16384, a + 24576, a + 28672            # 2x4x8 fp32 / 4x4x8 out: disjoint
    good = dict(image=img, labels=lab, channels=1, n_cls=3, src=(2, 4, 8), dst=(4, 4, 8), image_out=io, labels_out=lo,
                workspace=ws, workspace_bytes=4096)

    def call(**kw):
        k = {**good, **kw}
        return lib.hdf_resize_3d(k["image"], k["labels"], k["channels"], k["n_cls"], *k["src"], *k["dst"], k["image_out"],
                                 k["labels_out"], k["workspace"], k["workspace_bytes"], None)

    cases = {
        "no pair": dict(image=None, image_out=None, labels=None, labels_out=None),
        "image without image_out": dict(image_out=None),
        "image_out without image": dict(image=None),
        "labels without labels_out": dict(labels_out=None),
        "labels_out without labels": dict(labels=None),
        "a factor above 8": dict(src=(33, 4, 8), dst=(4, 4, 8)),
        "a factor above 8 on W": dict(src=(2, 4, 9), dst=(2, 4, 1)),
        "a dimension above 1024": dict(src=(2, 4, 1025)),
        "an output dimension above 1024": dict(dst=(4, 4, 1025)),
        "an empty axis": dict(src=(2, 0, 8)),
        "a negative axis": dict(dst=(4, -4, 8)),
        "one class": dict(n_cls=1),
        "nine classes": dict(n_cls=9),
        "65 channels": dict(channels=65),
        "negative channels": dict(channels=-1),
        "an image without channels": dict(channels=0),
        "a workspace too small": dict(src=(2, 4, 8), dst=(4, 8, 8), workspace_bytes=8 * 4 * 4 * 8 - 1),
        "a null workspace": dict(src=(2, 4, 8), dst=(4, 8, 8), workspace=None),
        "image_out is the image": dict(image_out=img),
        "labels_out is the labels": dict(labels_out=lab),
        "labels_out inside image_out": dict(labels_out=io + 16),
        "image_out overlaps the image's tail": dict(image_out=img + 4 * 63),
    }
    for what, kw in cases.items():
        rc = call(**kw)
        assert rc == 1 and lib.hdf_last_error().startswith(b"resize_3d:"), (what, rc, lib.hdf_last_error())
    for what, (n, lo_, hi_) in {"hi == lo": (8, 1.0, 1.0), "hi < lo": (8, 2.0, 1.0), "nan": (8, float("nan"), 1.0),
                                "inf": (8, 0.0, float("inf")), "overflowing range": (8, -3e38, 3e38),
                                "nothing": (0, 0.0, 1.0)}.items():
        rc = lib.hdf_trunc_normalize(a, n, lo_, hi_, None)
        assert rc == 1 and lib.hdf_last_error().startswith(b"trunc_normalize:"), (what, rc, lib.hdf_last_error())
    assert lib.hdf_trunc_normalize(None, 8, 0.0, 1.0, None) == 1
    assert not any(buf)                                                             # nothing was written through


def test_there_is_no_cpu_path():
    from hdf_rt import TrainTransform3D, _lib, crop_resize, resize_3d, trunc_normalize_
    image, labels = torch.zeros(1, 2, 4, 8), torch.zeros(2, 4, 8, dtype=torch.uint8)
    with pytest.raises(_lib.HdfError, match="no CPU path"):
        resize_3d(image, labels, 3, (4, 4, 8))
    with pytest.raises(_lib.HdfError, match="no CPU path"):
        resize_3d(None, labels, 3, (4, 4, 8))
    with pytest.raises(_lib.HdfError, match="no CPU path"):
        crop_resize(image, labels, 3, (4, 4, 8))
    with pytest.raises(_lib.HdfError, match="no CPU path"):
        trunc_normalize_(image, (-100, 200))
    with pytest.raises(_lib.HdfError, match="no CPU path"):
        TrainTransform3D.from_ids(3, [2, 3, 6], input_shape=(4, 4, 8))(image, labels)
