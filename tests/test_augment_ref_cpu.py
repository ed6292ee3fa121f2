"""The augmentation's yardstick, without a GPU: (a) tests/augment_ref.py agrees with scipy's map_coordinates in the mode a
current skimage.transform.warp uses; (b) the host-side draws of hdf_rt.augment follow the reference's closed forms and
draw order; (c) the checkers reject six planted defects at the shapes the GPU tests use; (d) augment_3d has no CPU path
and the C entry refuses a null matrix."""
import random

import numpy as np
import pytest
import torch

import augment_ref as ar
from hdf_rt import _lib
from hdf_rt.augment import TrainTransform3D, augment_3d, crop_origin, flip_flags, trz_matrix

C, NCLS = 3, 4


# ------------------------------------------------------------------------------------------------------ (a) vs scipy
@pytest.mark.parametrize("name", list(ar.MATRICES))
@pytest.mark.parametrize("blocky", [False, True], ids=["uniform", "blocky"])
def test_restatement_agrees_with_scipy_grid_constant(name, blocky):
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.RandomState(7)
    img = rng.standard_normal((C,) + ar.SHAPE)                       # unit scale: the bound below is absolute
    lab = ar.labels_of(ar.SHAPE, NCLS, 3, blocky)
    c = ar.source_coords(ar.SHAPE, ar.MATRICES[name])
    offs, wts = ar.corners(c, ar.SHAPE)

    def scipy_warp(vol):
        return ndi.map_coordinates(vol.astype(np.float64), c, order=1, mode="grid-constant", cval=0, prefilter=False,
                                   output=np.float64)

    for ch in img:
        assert np.abs(ar.interpolate(ch, offs, wts) - scipy_warp(ch)).max() <= 1e-12
    sums = ar.class_sums(lab, NCLS, offs, wts)
    for z in range(1, NCLS):
        assert np.abs(sums[z - 1] - scipy_warp(lab == z)).max() <= 1e-12
    # the condition check_labels puts on the inputs: no class sum within its 1e-7 band of 0.5, so nothing is excluded
    assert np.abs(sums - 0.5).min() > 1e-6, np.abs(sums - 0.5).min()


def test_grid_constant_differs_from_constant_where_the_issue_says():
    ndi = pytest.importorskip("scipy.ndimage")
    line = np.arange(1.0, 6.0)
    at = np.array([[-0.5]])
    assert ndi.map_coordinates(line, at, order=1, mode="grid-constant", cval=0, prefilter=False)[0] == 0.5
    assert ndi.map_coordinates(line, at, order=1, mode="constant", cval=0, prefilter=False)[0] == 0.0
    vol = line[None, None, :]
    c = np.array([0.0, 0.0, -0.5]).reshape(3, 1, 1, 1)
    offs, wts = ar.corners(c, vol.shape)
    assert ar.interpolate(vol, offs, wts)[0, 0, 0] == 0.5


# ------------------------------------------------------------------------------------------------- (b) host-side draws
@pytest.mark.parametrize("seed", [0, 1, 12345])
@pytest.mark.parametrize("mode", ["tr", "trz", "t", "r", "z", "rz", ""])
def test_trz_matrix_follows_the_closed_forms_and_the_draw_order(seed, mode):
    np.random.seed(seed)
    got = trz_matrix(mode)
    after = np.random.uniform(0, 1)
    np.random.seed(seed)
    t = [0, np.random.uniform(-5, 5), np.random.uniform(-5, 5)] if "t" in mode else [0, 0, 0]
    a = np.random.uniform(-5, 5) / 180.0 * np.pi if "r" in mode else 0.0
    z = [1, np.random.uniform(0.9, 1.1), np.random.uniform(0.9, 1.1)] if "z" in mode else [1, 1, 1]
    assert np.random.uniform(0, 1) == after                           # exactly the reference's number of draws
    rot = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    want = np.concatenate([rot @ np.diag(z), np.array(t, dtype=np.float64)[:, None]], 1)
    assert got.shape == (3, 4) and got.dtype == np.float64
    assert np.abs(got - want).max() <= 1e-15
    assert got[0].tolist() == [1.0, 0.0, 0.0, 0.0]                    # axis 0 is never moved


def test_mode_tr_consumes_exactly_three_uniforms_and_takes_an_rng():
    rs = np.random.RandomState(5)
    trz_matrix("tr", rs)
    ref = np.random.RandomState(5)
    ref.uniform(size=3)
    assert rs.uniform() == ref.uniform()
    np.random.seed(9)
    a = trz_matrix("tr")
    assert np.array_equal(a, trz_matrix("tr", np.random.RandomState(9)))


def test_flip_flags_always_flip_exactly_one_axis_in_mode_hv():
    np.random.seed(3)
    got = [flip_flags("hv") for _ in range(200)]
    np.random.seed(3)
    want = [np.random.uniform(0, 1) > 0.5 for _ in range(200)]
    assert [g[0] for g in got] == want and all(h != w for h, w in got)
    assert 50 < sum(want) < 150
    state = np.random.get_state()[1].copy()
    assert flip_flags("h") == (True, False) and flip_flags("v") == (False, True) and flip_flags("") == (False, False)
    assert np.array_equal(np.random.get_state()[1], state)            # no draw outside 'hv'


def test_crop_origin_stays_inside_and_draws_like_the_reference():
    shape, patch = (20, 45, 50), (16, 40, 50)
    random.seed(11)
    got = [crop_origin(shape, patch) for _ in range(300)]
    random.seed(11)
    want = [(random.randint(0, 4), random.randint(0, 5), 0) for _ in range(300)]
    assert got == want
    assert {g[0] for g in got} == set(range(5)) and {g[1] for g in got} == set(range(6))   # both ends are reached
    assert crop_origin((8, 8, 8), (16, 8, 4), random.Random(1))[:2] == (0, 0)


# ----------------------------------------------------------------------------------------- (c) planted defects rejected
def _planted(image, labels, n_cls, affine, flip_h, flip_w, defect):
    """tests/augment_ref.augment_ref with one defect: 'constant' border, 'gt' (> for >=), 'first' class wins,
    'flip_first', 'centre' (size - 1) / 2, 'fp32' image accumulation.  Returns (image fp32, labels)."""
    shape = labels.shape
    if defect == "flip_first":
        image, labels = ar.flip(image, flip_h, flip_w), ar.flip(labels, flip_h, flip_w)
    centre = [(n - 1) / 2 for n in shape] if defect == "centre" else None
    c = ar.source_coords(shape, affine, centre)
    offs, wts = ar.corners(c, shape)
    if defect == "constant":          # scipy's `constant`: exactly 0 outside [0, n-1]
        out = np.zeros(shape, dtype=bool)
        for a in range(3):
            out |= (c[a] < 0) | (c[a] > shape[a] - 1)
        wts = np.where(out[None], 0.0, wts)
    acc = np.float32 if defect == "fp32" else np.float64
    img = np.stack([ar.interpolate(ch, offs, wts, acc) for ch in image]).astype(np.float32)
    lab = ar.labels_from_sums(ar.class_sums(labels, n_cls, offs, wts), inclusive=defect != "gt",
                              last_wins=defect != "first")
    if defect != "flip_first":
        img, lab = ar.flip(img, flip_h, flip_w), ar.flip(lab, flip_h, flip_w)
    return img, lab


def _checked(image, labels, affine, flip_h, flip_w, defect, exact_labels):
    ref = ar.augment_ref(image, labels, NCLS, affine, flip_h, flip_w)
    img, lab = _planted(image, labels, NCLS, affine, flip_h, flip_w, defect)
    for ch in range(image.shape[0]):
        ar.check_image(img[ch], ref["image"][ch], np.abs(image[ch]).max())
    if exact_labels:
        ar.check_exact(lab, ref["labels"], "labels")
    else:
        ar.check_labels(lab, ref["sums"])


HALF = ar.translation((0, 0.5, 0))


def test_the_checkers_accept_the_restatement_itself():
    image, labels = ar.image_of(ar.SHAPE, C, 1), ar.labels_of(ar.SHAPE, NCLS, 1)
    _checked(image, labels, ar.TR, True, False, None, False)
    _checked(image, labels, HALF, False, False, None, True)


@pytest.mark.parametrize("defect,affine,flip_h,exact", [
    ("constant", ar.TR, False, False), ("gt", HALF, False, True), ("first", HALF, False, True),
    ("flip_first", ar.TR, True, False), ("centre", ar.TR, False, False), ("fp32", ar.TR, False, False)],
    ids=["constant-border", "gt-for-ge", "first-class-wins", "flip-before-warp", "centre-size-minus-1", "fp32-sum"])
def test_the_checkers_reject_a_planted_defect(defect, affine, flip_h, exact):
    image, labels = ar.image_of(ar.SHAPE, C, 1), ar.labels_of(ar.SHAPE, NCLS, 1)
    with pytest.raises(AssertionError):
        _checked(image, labels, affine, flip_h, False, defect, exact)


def test_half_voxel_translation_has_thousands_of_exact_halves():
    labels = ar.labels_of(ar.SHAPE, NCLS, 1)
    sums = ar.augment_ref(ar.image_of(ar.SHAPE, 1, 1), labels, NCLS, HALF)["sums"]
    assert set(np.unique(sums)) <= {0.0, 0.5, 1.0}
    assert int((sums == 0.5).sum()) > 5000
    assert int(((sums == 0.5).sum(0) == 2).sum()) > 500               # two classes at 1/2: last-class-wins decides
    assert int((((sums == 0.5).sum(0) == 1) & (sums.sum(0) == 0.5)).sum()) > 500   # a class against background at 1/2


# ------------------------------------------------------------------------------------------------------- (d) no CPU path
def test_augment_3d_fails_loudly_without_a_gpu():
    image, labels = torch.zeros(2, 4, 5, 6), torch.zeros(4, 5, 6, dtype=torch.uint8)
    with pytest.raises(_lib.HdfError, match="no CPU path"):
        augment_3d(image, labels, 3, ar.IDENTITY)
    with pytest.raises(_lib.HdfError, match="no CPU path"):
        TrainTransform3D(3, patch_size=(4, 4, 4))(image, labels)
    assert "hdf_augment_3d" in _lib.EXPORTS


def test_entry_refuses_a_null_affine_on_the_host():
    """the one refusal that can be provoked without a device: the matrix is a HOST pointer, checked before the arguments
    reach the launcher, so no device address is needed and nothing can launch.  Every other refusal is exercised with real
    device buffers in tests/test_gpu_augment.py."""
    lib = _lib.lib()
    rc = lib.hdf_augment_3d(None, None, 2, 3, 2, 3, 4, None, 1, 0, None, None, None, None)
    assert rc == 1 and lib.hdf_last_error().startswith(b"augment_3d: null affine"), (rc, lib.hdf_last_error())
