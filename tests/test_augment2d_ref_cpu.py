"""The 2-D augmentation's yardstick, without a GPU.  The contract of hdf_augment_2d (include/hdf.h) is EXACT, so every
comparison here is of bits: (a) tests/augment2d_ref.py equals what PIL 12.2.0 recorded in tests/golden/augment2d_pil.npz
(always runs) and a live PIL where one is importable -- including 0, 90, 180 and 270 degrees, which PIL short-cuts to
copies and transposes while the restatement (and the kernel) take the general path; (b) check_exact rejects four planted
defects; (c) the host side of hdf_rt.augment -- rotate_matrix, rotate_degree, flip2d_code -- builds PIL's matrix and
follows the reference's draws; (d) the C entry is exported as declared, refuses null host arrays, and there is no CPU
path."""
import ctypes
import math
import os
import random

import numpy as np
import pytest
import torch

import augment2d_ref as ar
from hdf_rt import _lib
from hdf_rt.augment import TrainTransform2D, augment_2d, flip2d_code, rotate_degree, rotate_matrix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "augment2d_pil.npz"))
N_GOLDEN = len(GOLDEN["cases"])


# ---------------------------------------------------------------------------------------------------------- (a) vs PIL
@pytest.mark.parametrize("k", range(N_GOLDEN))
def test_restatement_equals_the_recorded_pil_output(k):
    h, w, angle = GOLDEN["cases"][k]
    h, w = int(h), int(w)
    image, labels = GOLDEN["image_%d" % k], GOLDEN["labels_%d" % k]
    assert image.shape == (len(ar.SCALES), h, w) and image.dtype == np.float32 and labels.dtype == np.uint8
    m = ar.matrix_of(float(angle), w, h)
    for ch in range(image.shape[0]):
        ar.check_exact(ar.rotate_image(image[ch], m), GOLDEN["pil_image_%d" % k][ch], "image %d" % ch)
    ar.check_exact(ar.rotate_labels(labels, m), GOLDEN["pil_labels_%d" % k], "labels")


def test_the_fixture_covers_what_it_should():
    cases = [tuple(c) for c in GOLDEN["cases"]]
    assert 12 <= len(cases) <= 16
    assert {(int(h), int(w)) for h, w, _ in cases} == set(ar.SHAPES)
    angles = {a for _, _, a in cases}
    assert {0, 90, 180, 270, 37.3, 181} <= angles and any(a < 0 for a in angles)
    assert str(GOLDEN["pil_version"]) == "12.2.0"
    seen = set()
    for k in range(len(cases)):
        seen |= set(np.unique(GOLDEN["labels_%d" % k]).tolist())
        assert (GOLDEN["pil_image_%d" % k] != 0).any()
    assert {0, 1, 2, 3, 200, 255} <= seen


@pytest.mark.parametrize("shape", ar.SHAPES, ids=lambda s: "%dx%d" % s)
def test_restatement_equals_live_pil(shape):
    image_mod = pytest.importorskip("PIL.Image")
    labels = ar.labels_of(shape, 3)
    if labels.size >= 6:
        assert {0, 1, 2, 3, 200, 255} <= set(np.unique(labels).tolist())
    images = [ar.image_of(shape, 1, 5, s)[0] for s in ar.SCALES]
    for angle in ar.ANGLES:
        m = ar.matrix_of(angle, shape[1], shape[0])
        want = np.array(image_mod.fromarray(labels).rotate(angle, image_mod.NEAREST))
        ar.check_exact(ar.rotate_labels(labels, m), want, "labels at %s degrees" % angle)
        for scale, img in zip(ar.SCALES, images):
            want = np.array(image_mod.fromarray(img).rotate(angle, image_mod.BILINEAR))
            ar.check_exact(ar.rotate_image(img, m), want, "image x %g at %s degrees" % (scale, angle))


# ----------------------------------------------------------------------------------------- (b) planted defects rejected
DEFECT_ANGLES = (-15, -10, -5, 5, 10, 15)


def _planted(image, labels, angle, flip_code, defect):
    """the restatement with one defect: 'fp64_diff' (the neighbour difference in fp64), 'centre' ((size - 1) / 2),
    'flip_first', 'floor_label' (the nearest label at the floor of the fp64 coordinate).  Returns (image, labels)."""
    h, w = labels.shape
    m = ar.matrix_of(angle, w, h, centre=((w - 1) / 2.0, (h - 1) / 2.0) if defect == "centre" else None)
    if defect == "flip_first":
        image, labels = ar.flip(image, flip_code), ar.flip(labels, flip_code)
    img = np.stack([ar.rotate_image(ch, m, np.float64 if defect == "fp64_diff" else np.float32) for ch in image])
    lab = ar.rotate_labels(labels, m, floor_of_fp64=defect == "floor_label")
    if defect != "flip_first":
        img, lab = ar.flip(img, flip_code), ar.flip(lab, flip_code)
    return img, lab


def _checked(shape, flip_code, defect, what, blocky=True):
    """every reference angle but 0 at one shape, image or labels against the restatement"""
    image, labels = ar.image_of(shape, 2, 1), ar.labels_of(shape, 1, blocky)
    for angle in DEFECT_ANGLES:
        ref = ar.augment2d_ref(image, labels, 4, ar.matrix_of(angle, shape[1], shape[0]), flip_code)
        img, lab = _planted(image, labels, angle, flip_code, defect)
        if what == "image":
            ar.check_exact(img, ref["image"], "image")
        else:
            ar.check_exact(lab, ref["labels"], "labels")


def test_the_checker_accepts_the_restatement_itself():
    for what in ("image", "labels"):
        _checked((24, 24), 0, None, what)
        _checked((17, 29), 1, None, what)
        _checked((37, 43), 0, None, what, blocky=False)


@pytest.mark.parametrize("defect,shape,flip_code,what", [
    ("fp64_diff", (24, 24), 0, "image"), ("centre", (24, 24), 0, "image"), ("centre", (24, 24), 0, "labels"),
    ("flip_first", (17, 29), 1, "image"), ("flip_first", (17, 29), 2, "labels"), ("floor_label", (37, 43), 0, "labels")],
    ids=["fp64-difference", "centre-image", "centre-labels", "flip-first-image", "flip-first-labels", "floor-label"])
def test_the_checker_rejects_a_planted_defect(defect, shape, flip_code, what):
    """floor-label: the floor of the fp64 coordinate and the 16.16 index part only where a coordinate lies within 2^-17
    of an integer.  Over the reference's angles that is NO pixel at 24x24, 17x29, 1x9, 9x1 and 2x2 -- the defect is
    indistinguishable there --, one pixel at 40x33 (-10 degrees) and one each at 37x43 for -5 and +5 degrees (1755 over
    the twelve angles at 384x384).  So this case runs at 37x43 with labels that change from pixel to pixel, where that
    one pixel carries another byte."""
    with pytest.raises(AssertionError, match="differ"):
        _checked(shape, flip_code, defect, what, blocky=defect != "floor_label")


# ------------------------------------------------------------------------------------------------- (c) the host side
def _pil_matrix(image_mod, monkeypatch, angle, width, height):
    """the matrix Image.rotate hands to Image.transform, or None where rotate short-cuts to a copy or a transpose"""
    seen = []
    real = image_mod.Image.transform

    def spy(self, size, method, data=None, *args, **kwargs):
        seen.append(tuple(data))
        return real(self, size, method, data, *args, **kwargs)

    with monkeypatch.context() as mp:
        mp.setattr(image_mod.Image, "transform", spy)
        image_mod.new("F", (width, height)).rotate(angle, image_mod.BILINEAR)
    return seen[0] if seen else None


def test_rotate_matrix_is_the_matrix_pil_builds(monkeypatch):
    image_mod = pytest.importorskip("PIL.Image")
    general = 0
    for h, w in ar.SHAPES:
        for angle in ar.ANGLES:
            got = rotate_matrix(angle, w, h)
            assert got == ar.matrix_of(angle, w, h)
            want = _pil_matrix(image_mod, monkeypatch, angle, w, h)
            if want is None:
                assert angle in (0, 180) or (angle in (90, 270) and h == w), (angle, h, w)
            else:
                general += 1
                assert got == want, (angle, h, w, got, want)
    assert general >= 60


def test_rotate_matrix_without_pil():
    for h, w in ar.SHAPES:
        for angle in ar.ANGLES:
            got = rotate_matrix(angle, w, h)
            assert len(got) == 6 and all(type(v) is float for v in got)
            assert got == ar.matrix_of(angle, w, h) and ar.passes_check_fixed(got, w, h)
    assert rotate_matrix(0, 43, 37) == ar.IDENTITY
    assert rotate_matrix(180, 43, 37) == (-1.0, 0.0, 43.0, 0.0, -1.0, 37.0)
    a, b, c, d, e, f = rotate_matrix(10, 43, 37)
    assert a == e == round(math.cos(math.radians(10)), 15) and d == -b == round(math.sin(math.radians(10)), 15)


@pytest.mark.parametrize("seed", [0, 1, 12345])
def test_rotate_degree_draws_like_random_rotate_2d(seed):
    degree = [-15, -10, -5, 0, 5, 10, 15]                             # transformer_2d.py:144
    random.seed(seed)
    got = [rotate_degree() for _ in range(100)]
    after = random.random()
    random.seed(seed)
    want = [random.choice(degree) for _ in range(100)]                # :161
    assert got == want and random.random() == after
    assert set(got) == set(degree)
    assert rotate_degree((90,), random.Random(3)) == 90
    assert rotate_degree((1, 2, 3), random.Random(7)) == random.Random(7).choice([1, 2, 3])      # takes an rng


@pytest.mark.parametrize("seed", [0, 1, 12345])
@pytest.mark.parametrize("mode", ["hv", "h", "v", ""])
def test_flip2d_code_draws_like_random_flip_2d(seed, mode):
    np.random.seed(seed)
    got = [flip2d_code(mode) for _ in range(300)]
    after = np.random.uniform(0, 1)
    np.random.seed(seed)
    want = []
    for _ in range(300):                                              # transformer_2d.py:99-128 restated
        code = 0
        if "h" in mode and "v" in mode:
            random_factor = np.random.uniform(0, 1)
            if random_factor < 0.3:
                code = 1                                              # [:, ::-1]: W
            elif random_factor < 0.6:
                code = 2                                              # [::-1, :]: H
        elif "h" in mode:
            if np.random.uniform(0, 1) > 0.5:
                code = 1
        elif "v" in mode:
            if np.random.uniform(0, 1) > 0.5:
                code = 2
        want.append(code)
    assert got == want and np.random.uniform(0, 1) == after          # exactly the reference's number of draws
    assert set(got) == {"hv": {0, 1, 2}, "h": {0, 1}, "v": {0, 2}, "": {0}}[mode]
    rs = np.random.RandomState(seed)
    np.random.seed(seed)
    assert [flip2d_code(mode, rs) for _ in range(20)] == [flip2d_code(mode) for _ in range(20)]


# ------------------------------------------------------------------------------------------- (d) the entry, no CPU path
def test_the_symbol_is_exported_with_the_declared_signature():
    hdr = " ".join(open(os.path.join(ROOT, "include", "hdf.h")).read().split())
    decl = ("int hdf_augment_2d(const float* image, const uint8_t* labels, int batch, int channels, int n_cls, int H, "
            "int W, const double* matrices, const uint8_t* flips, float* image_out, uint8_t* labels_out, "
            "float* onehot_out, hdf_stream stream);")
    assert decl in hdr
    assert "hdf_augment_2d" in _lib.EXPORTS
    fn = _lib.lib().hdf_augment_2d
    vp, i = ctypes.c_void_p, ctypes.c_int
    assert fn.restype is i
    assert list(fn.argtypes) == [vp, vp, i, i, i, i, i, ctypes.POINTER(ctypes.c_double), vp, vp, vp, vp, vp]
    import hdf_rt
    for name in ("TrainTransform2D", "augment_2d", "flip2d_code", "rotate_degree", "rotate_matrix"):
        assert name in dir(hdf_rt) and getattr(hdf_rt, name) is getattr(hdf_rt.augment, name)


def test_entry_refuses_null_host_arrays():
    """the refusals that can be provoked without a device: matrices and flips are HOST pointers, checked before anything
    else, so no device address is needed and nothing can launch.  Every other refusal is exercised with real device
    buffers in tests/test_gpu_augment2d.py."""
    lib = _lib.lib()
    mats = np.array([ar.IDENTITY], dtype=np.float64)
    flips = np.zeros(1, dtype=np.uint8)
    rc = lib.hdf_augment_2d(None, None, 1, 2, 3, 4, 5, None, flips.ctypes.data, None, None, None, None)
    assert rc == 1 and lib.hdf_last_error().startswith(b"augment_2d: null matrices"), (rc, lib.hdf_last_error())
    rc = lib.hdf_augment_2d(None, None, 1, 2, 3, 4, 5, mats.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), None, None,
                            None, None, None)
    assert rc == 1 and lib.hdf_last_error().startswith(b"augment_2d: null flips"), (rc, lib.hdf_last_error())


def test_augment_2d_fails_loudly_without_a_gpu():
    image, labels = torch.zeros(2, 2, 5, 6), torch.zeros(2, 5, 6, dtype=torch.uint8)
    with pytest.raises(_lib.HdfError, match="no CPU path"):
        augment_2d(image, labels, 3, [ar.IDENTITY] * 2, [0, 0])
    with pytest.raises(_lib.HdfError, match="no CPU path"):
        TrainTransform2D(3)(image, labels)
    with pytest.raises(ValueError, match="normalize"):
        TrainTransform2D(3, normalize="petct")
