"""The yardstick of the 2-D erase / zoom / gamma / noise transforms, without a GPU.  The contract of hdf_zoom_2d
(include/hdf.h) is EXACT, so every comparison of a resampled plane here is of bits: (a) tests/zoom2d_ref.py equals what
PIL 12.2.0 recorded in tests/golden/zoom2d_pil.npz from real crop / ImageOps.expand / resize calls (always runs) and a live
PIL where one is importable; (b) check_exact rejects four planted defects; (c) the host side of hdf_rt.augment --
erase2d_keep, zoom2d_canvas, gamma2d, noise2d_flag, TrainTransform2D.draw and from_ids -- follows the reference's draws,
checked against hand-worked cases; (d) the C entries are exported as declared, refuse null arrays, and there is no CPU
path."""
import ctypes
import hashlib
import os
import random

import numpy as np
import pytest
import torch

import zoom2d_ref as zr
from hdf_rt import _lib
from hdf_rt.augment import (REFERENCE_DEGREES, TrainTransform2D, erase2d_keep, gamma2d, intensity_2d_, label_bbox_2d,
                            noise2d_flag, zoom2d_canvas, zoom_2d)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "zoom2d_pil.npz"))
CASES = [tuple(c) for c in GOLDEN["cases"]]


def _case(k):
    h, w, factor, x1, y1, p0, p1 = CASES[k]
    return (int(h), int(w)), float(factor), (int(x1), int(y1), int(p0), int(p1))


def _inputs(k, shape):
    """as tools/make_zoom2d_golden.py builds them"""
    image = np.concatenate([zr.image_of(shape, 1, 40 + k, s) for s in zr.SCALES])
    return image, zr.labels_of(shape, 40 + k, blocky=False)


def _digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# ---------------------------------------------------------------------------------------------------------- (a) vs PIL
@pytest.mark.parametrize("shape", zr.SHAPES, ids=lambda s: "%dx%d" % s)
def test_restatement_equals_the_recorded_pil_output(shape):
    ks = [k for k in range(len(CASES)) if _case(k)[0] == shape]
    assert len(ks) >= 2 * len(zr.FACTORS)
    for k in ks:
        _, factor, draws = _case(k)
        image, labels = _inputs(k, shape)
        canvas = tuple(int(v) for v in GOLDEN["canvases"][k])
        h, w = shape
        tw, th = int(w * factor), int(h * factor)
        assert canvas == (zr.crop_canvas(draws[0], draws[1], tw, th) if factor < 1.0
                          else zr.expand_canvas(draws[2], draws[3], tw, th)), (k, canvas)
        got_i = zr.zoom_image(image, zr.full_keep(h, w), canvas)
        got_l = zr.zoom_labels(labels, canvas)
        what = "case %d: %dx%d factor %g draws %s" % ((k,) + shape + (factor, draws))
        if "pil_image_%d" % k in GOLDEN:                              # the arrays themselves: a mismatch is located
            zr.check_exact(got_i, GOLDEN["pil_image_%d" % k], what + " image")
            zr.check_exact(got_l, GOLDEN["pil_labels_%d" % k], what + " labels")
        assert _digest(got_i) == str(GOLDEN["sha_image"][k]), what + " image"
        assert _digest(got_l) == str(GOLDEN["sha_labels"][k]), what + " labels"


def test_the_fixture_covers_what_it_should():
    assert str(GOLDEN["pil_version"]) == "12.2.0"
    assert {(int(h), int(w)) for h, w, *_ in CASES} == set(zr.SHAPES)
    for shape in zr.SHAPES:
        assert {c[2] for c in CASES if (int(c[0]), int(c[1])) == shape} == set(zr.FACTORS)
    off_plane = skipped = shrunk = grown = 0
    for k in range(len(CASES)):
        (h, w), factor, (x1, y1, _, _) = _case(k)
        sw, sh, ox, oy = (int(v) for v in GOLDEN["canvases"][k])
        off_plane += factor < 1.0 and (x1 < 0 or y1 < 0 or x1 + sw > w or y1 + sh > h)
        skipped += (sw, sh) == (w, h)
        shrunk += sw > w
        grown += sw < w
        assert (sw, sh) != (w, h) or (ox, oy) == (0, 0)
    assert off_plane >= 2 * len(zr.SHAPES) and skipped >= len(zr.SHAPES) and shrunk and grown
    assert sum("pil_image_%d" % k in GOLDEN for k in range(len(CASES))) >= 2 * len(zr.FACTORS)
    image, labels = _inputs(0, zr.SHAPES[0])
    assert {0, 1, 2, 3, 200, 255} <= set(np.unique(labels).tolist())
    assert abs(float(np.abs(image[1]).max()) / float(np.abs(image[0]).max()) - 1000.0) < 500.0   # scales 1 and 1000


@pytest.mark.parametrize("shape", zr.SHAPES, ids=lambda s: "%dx%d" % s)
def test_restatement_equals_live_pil(shape):
    pytest.importorskip("PIL.Image")
    h, w = shape
    labels = zr.labels_of(shape, 3, blocky=False)
    images = [zr.image_of(shape, 1, 5, s)[0] for s in zr.SCALES]
    for factor in zr.FACTORS:
        for draws in zr.zoom_cases(shape, factor):
            want, canvas = zr.pil_zoom(labels, factor, *draws)
            zr.check_exact(zr.zoom_labels(labels, canvas), want, "labels x %g %s" % (factor, draws))
            for scale, img in zip(zr.SCALES, images):
                want, canvas = zr.pil_zoom(img, factor, *draws)
                got = zr.zoom_image(img[None], zr.full_keep(h, w), canvas)[0]
                zr.check_exact(got, want, "image x %g at factor %g %s" % (scale, factor, draws))


# ----------------------------------------------------------------------------------------- (b) planted defects rejected
def _defect_case(name):
    """(shape, keep, canvas) at which the planted defect shows"""
    if name == "closed_form":
        return (40, 40), zr.full_keep(40, 40), zr.expand_canvas(0, 0, 48, 48)     # 48 -> 40: four indices differ
    if name == "erase_last":
        return (37, 43), (5, 37, 0, 40), zr.crop_canvas(3, 2, 34, 29)
    if name == "widen":
        return (37, 43), zr.full_keep(37, 43), zr.expand_canvas(2, 1, 51, 44)     # shrinking: the support widens
    return (37, 43), zr.full_keep(37, 43), zr.crop_canvas(3, 2, 34, 29)           # both passes run


def _planted(name):
    shape, keep, canvas = _defect_case(name)
    image, labels = zr.image_of(shape, 2, 1), zr.labels_of(shape, 1, blocky=False)
    ref_i, ref_l = zr.zoom_image(image, keep, canvas), zr.zoom_labels(labels, canvas)
    if name == "closed_form":
        zr.check_exact(zr.zoom_labels(labels, canvas, closed_form=True), ref_l, "labels")
    elif name == "erase_last":
        zr.check_exact(zr.zoom_image(image, keep, canvas, erase_last=True), ref_i, "image")
    elif name == "widen":
        zr.check_exact(zr.zoom_image(image, keep, canvas, widen=False), ref_i, "image")
    elif name == "fp64_intermediate":
        zr.check_exact(zr.zoom_image(image, keep, canvas, fp64_intermediate=True), ref_i, "image")
    else:
        zr.check_exact(zr.zoom_image(image, keep, canvas), ref_i, "image")
        zr.check_exact(zr.zoom_labels(labels, canvas), ref_l, "labels")


def test_the_checker_accepts_the_restatement_itself():
    for name in ("closed_form", "erase_last", "widen", "fp64_intermediate"):
        shape, keep, canvas = _defect_case(name)
        image = zr.image_of(shape, 2, 1)
        zr.check_exact(zr.zoom_image(image, keep, canvas), zr.zoom_image(image, keep, canvas), name)
    _planted(None)


@pytest.mark.parametrize("name", ["fp64_intermediate", "closed_form", "widen", "erase_last"])
def test_the_checker_rejects_a_planted_defect(name):
    """fp64_intermediate: the horizontal result kept in fp64; closed_form: the nearest index as (int)((x + 0.5) a0)
    instead of the running sum (they part at 48 -> 40, not at 40 -> 48); widen: the support kept at 1 when shrinking;
    erase_last: the erase applied after the resample"""
    with pytest.raises(AssertionError, match="differ"):
        _planted(name)


def test_running_sum_and_closed_form_part_where_claimed():
    assert int((zr.nearest_table(48, 40) != zr.nearest_table(48, 40, closed_form=True)).sum()) == 4
    assert np.array_equal(zr.nearest_table(40, 48), zr.nearest_table(40, 48, closed_form=True))
    assert np.array_equal(zr.nearest_table(37, 37), np.arange(37))


# ------------------------------------------------------------------------------------------------- (c) the host side
class Script:
    """an rng that returns scripted values and records every call, so the order and the arguments are checked"""

    def __init__(self, *values):
        self.values, self.calls = list(values), []

    def _next(self, name, *args):
        self.calls.append((name,) + args)
        return self.values.pop(0)

    def randint(self, a, b):
        v = self._next("randint", a, b)
        assert a <= v <= b
        return v

    def uniform(self, a, b):
        return self._next("uniform", a, b)

    def choice(self, seq):
        v = self._next("choice", tuple(seq))
        assert v in seq
        return v


DIRECTIONS = ("t", "d", "l", "r", "no_erase")
EMPTY_48 = (0, 48, -1, 48, -1)
FOUR_DRAWS = [("randint", 0, 64), ("randint", -64, 0), ("randint", 0, 64), ("randint", -64, 0), ("choice", DIRECTIONS)]


@pytest.mark.parametrize("draws,direction,keep", [
    ((10, -20, 7, -5), "t", (10, 48, 0, 48)),           # rows [:10] zeroed
    ((10, -20, 7, -5), "d", (0, 28, 0, 48)),            # rows [-20:] zeroed: a negative value counts from the end
    ((10, -20, 7, -5), "l", (0, 48, 7, 48)),
    ((10, -20, 7, -5), "r", (0, 48, 0, 43)),
    ((10, -20, 7, -5), "no_erase", (0, 48, 0, 48)),
    ((10, 0, 7, -5), "d", (0, 0, 0, 48)),               # rows [0:]: a drawn 0 erases the whole plane
    ((10, -20, 7, 0), "r", (0, 48, 0, 0)),
    ((64, -20, 7, -5), "t", (48, 48, 0, 48)),           # rows [:64] of 48: everything
    ((0, -64, 0, -64), "t", (0, 48, 0, 48)),            # rows [:0]: nothing
    ((0, -64, 0, -64), "d", (0, 0, 0, 48)),             # rows [-64:] of 48: everything
])
def test_erase_of_an_empty_label(draws, direction, keep):
    rng = Script(*draws, direction)
    assert erase2d_keep(EMPTY_48, 48, 48, rng=rng) == keep
    assert rng.calls == FOUR_DRAWS and not rng.values


@pytest.mark.parametrize("bbox,direction,keep", [
    ((4, 0, 1, 0, 1), "t", (0, 48, 0, 48)),             # a box at the corner: rw0 = (0, 33), rows [:0] is nothing
    ((4, 0, 1, 0, 1), "d", (0, 33, 0, 48)),
    ((4, 0, 1, 0, 1), "r", (0, 48, 0, 33)),
    ((4, 46, 47, 46, 47), "t", (14, 48, 0, 48)),        # the far corner: rw0 = (14, 48), rows [48:] is nothing
    ((4, 46, 47, 46, 47), "d", (0, 48, 0, 48)),
    ((4, 46, 47, 46, 47), "l", (0, 48, 14, 48)),
    ((9, 20, 22, 10, 12), "r", (0, 48, 0, 44)),
    ((9, 20, 22, 10, 12), "t", (0, 48, 0, 48)),         # max(20 - 32, 0) = 0
])
def test_erase_around_a_label(bbox, direction, keep):
    rng = Script(direction)
    assert erase2d_keep(bbox, 48, 48, rng=rng) == keep
    assert rng.calls == [("choice", DIRECTIONS)]         # no draw for the window
    rng = Script("d")
    assert erase2d_keep((9, 20, 22, 10, 12), 48, 48, window=(8, 8), rng=rng) == (0, 26, 0, 48)


def test_zoom_crop_of_an_empty_label_keeps_the_swapped_names():
    """37x43 at 0.8: tw = int(43 * 0.8) = 34, th = int(37 * 0.8) = 29; the column is drawn in [0, W - th] = [0, 14] and
    the row in [0, H - tw] = [0, 3], so a crop 34 wide may start at column 14 and leave the 43 columns"""
    rng = Script(0.8, 14, 3)
    assert zoom2d_canvas((0, 37, -1, 43, -1), 37, 43, rng=rng) == (34, 29, -14, -3)
    assert rng.calls == [("uniform", 0.8, 1.2), ("randint", 0, 14), ("randint", 0, 3)]


def test_zoom_crop_around_a_label():
    rng = Script(0.8, 0, 0)                              # a box at the corner of 48x48: tw = th = 38
    assert zoom2d_canvas((4, 0, 1, 0, 1), 48, 48, rng=rng) == (38, 38, 0, 0)
    assert rng.calls == [("uniform", 0.8, 1.2), ("randint", 0, 0), ("randint", 0, 0)]
    # rows 30..40, columns 5..20: x1 in [max(0, min(5, 20 - 38)), min(5, 10)] = [0, 5], then y1 in [max(0, min(30,
    # 40 - 38)), min(30, 10)] = [2, 10]
    rng = Script(0.8, 5, 2)
    assert zoom2d_canvas((50, 30, 40, 5, 20), 48, 48, rng=rng) == (38, 38, -5, -2)
    assert rng.calls == [("uniform", 0.8, 1.2), ("randint", 0, 5), ("randint", 2, 10)]
    # and on 37x43 the swap again: rows 10..12, columns 30..33: x1 in [max(0, min(30, 33 - 29)), min(30, 43 - 29)] =
    # [4, 14], y1 in [max(0, min(10, 12 - 34)), min(10, 37 - 34)] = [0, 3]
    rng = Script(0.8, 9, 1)
    assert zoom2d_canvas((6, 10, 12, 30, 33), 37, 43, rng=rng) == (34, 29, -9, -1)
    assert rng.calls == [("uniform", 0.8, 1.2), ("randint", 4, 14), ("randint", 0, 3)]


def test_zoom_raises_value_error_on_an_empty_range_like_the_reference():
    """43x37 at 0.9: th = int(43 * 0.9) = 38 exceeds W = 37, so the column range is [0, -1]"""
    with pytest.raises(ValueError):
        zoom2d_canvas((0, 43, -1, 37, -1), 43, 37, scale=(0.9, 0.9), rng=random.Random(1))


def test_zoom_pad():
    rng = Script(1.2, 3.7, 0.4)                          # 48x48: tw = th = 57, both pads below (57 - 48) / 2
    assert zoom2d_canvas(EMPTY_48, 48, 48, rng=rng) == (60, 57, 3, 0)
    assert rng.calls == [("uniform", 0.8, 1.2), ("uniform", 0, 4.5), ("uniform", 0, 4.5)]
    rng = Script(1.0, 0.0, 0.0)                          # factor 1: nothing moves, the resize is skipped
    assert zoom2d_canvas(EMPTY_48, 48, 48, rng=rng) == (48, 48, 0, 0)
    # 37x43, the reference's `tw - w` and `th - h` with w the height and h the width: tw = 51, th = 44, pads below
    # (51 - 37) / 2 = 7 and (44 - 43) / 2 = 0.5, borders (6, 0, 14, 1): 6 + 43 + 14 = 63 wide, 0 + 37 + 1 = 38 high
    rng = Script(1.2, 6.9, 0.3)
    assert zoom2d_canvas((0, 37, -1, 43, -1), 37, 43, rng=rng) == (63, 38, 6, 0)
    assert rng.calls == [("uniform", 0.8, 1.2), ("uniform", 0, 7.0), ("uniform", 0, 0.5)]


def test_gamma_and_noise_draw_once_each():
    rng = Script(0.93)
    assert gamma2d(rng=rng) == 0.93 and rng.calls == [("uniform", 0.8, 1.2)]
    rng = Script(0.9, 0.9000001)
    assert noise2d_flag(rng) is False and noise2d_flag(rng) is True       # above 0.9, not at it
    assert rng.calls == [("uniform", 0, 1)] * 2


@pytest.mark.parametrize("seed", [0, 1, 12345])
def test_helpers_draw_in_the_references_order_under_a_seeded_random(seed):
    random.seed(seed)
    got = (erase2d_keep(EMPTY_48, 48, 48), zoom2d_canvas(EMPTY_48, 48, 48), gamma2d(), noise2d_flag())
    after = random.random()
    random.seed(seed)
    rw = [random.randint(0, 64), random.randint(-64, 0), random.randint(0, 64), random.randint(-64, 0)]
    direction = random.choice(["t", "d", "l", "r", "no_erase"])
    s = random.uniform(0.8, 1.2)
    t = int(48 * s)
    if s < 1.0:
        x1 = random.randint(0, 48 - t)
        y1 = random.randint(0, 48 - t)
        canvas = (t, t, -x1, -y1)
    else:
        p0 = int(random.uniform(0, (t - 48) / 2))
        p1 = int(random.uniform(0, (t - 48) / 2))
        canvas = (t + p0, t + p1, p0, p1)
    g, flag = random.uniform(0.8, 1.2), random.uniform(0, 1) > 0.9
    keep = {"t": (min(rw[0], 48), 48, 0, 48), "d": (0, max(48 + rw[1], 0) if rw[1] else 0, 0, 48),
            "l": (0, 48, min(rw[2], 48), 48), "r": (0, 48, 0, max(48 + rw[3], 0) if rw[3] else 0),
            "no_erase": (0, 48, 0, 48)}[direction]
    assert got == (keep, canvas, g, flag) and random.random() == after


def test_default_chain_consumes_exactly_the_draws_it_did():
    """TrainTransform2D(n_cls) with no new keyword: per sample one random.choice of the degree, then one np.random
    uniform for the flip, nothing else -- in particular no seed for a noise that is off"""
    tf = TrainTransform2D(3)
    assert (tf.erase, tf.zoom, tf.gamma, tf.noise) == (None, None, None, False)
    random.seed(3), np.random.seed(3)
    d = tf.draw(5, 17, 29)
    after = (random.random(), np.random.uniform(0, 1))
    random.seed(3), np.random.seed(3)
    degrees, us = [], []
    for _ in range(5):
        degrees.append(random.choice(list(REFERENCE_DEGREES)))
        us.append(np.random.uniform(0, 1))
    assert (random.random(), np.random.uniform(0, 1)) == after
    from hdf_rt.augment import rotate_matrix
    assert d["matrices"] == [rotate_matrix(a, 29, 17) for a in degrees]
    assert d["flips"] == [1 if u < 0.3 else 2 if u < 0.6 else 0 for u in us]
    assert d["keeps"] == [(0, 17, 0, 29)] * 5 and d["canvases"] == [(29, 17, 0, 0)] * 5
    assert d["gammas"] == [1.0] * 5 and d["noise"] == [0] * 5 and d["seed"] == 0


def test_full_chain_draws_erase_zoom_rotate_flip_gamma_noise_then_one_seed():
    tf = TrainTransform2D.from_ids(2, [1, 3, 4, 6, 7, 8, 9, 10])
    bbox = np.array([EMPTY_48, (9, 20, 22, 10, 12), EMPTY_48], dtype=np.int32)
    random.seed(8), np.random.seed(8)
    d = tf.draw(3, 48, 48, bbox)
    after = (random.random(), np.random.uniform(0, 1))
    random.seed(8), np.random.seed(8)
    from hdf_rt.augment import flip2d_code, rotate_degree, rotate_matrix
    want = {k: [] for k in ("keeps", "canvases", "matrices", "flips", "gammas", "noise")}
    for k in range(3):
        want["keeps"].append(erase2d_keep(bbox[k], 48, 48))
        want["canvases"].append(zoom2d_canvas(bbox[k], 48, 48))
        want["matrices"].append(rotate_matrix(rotate_degree(), 48, 48))
        want["flips"].append(flip2d_code("hv"))
        want["gammas"].append(gamma2d())
        want["noise"].append(int(noise2d_flag()))
    want["seed"] = int(np.random.randint(0, 2 ** 63 - 1, dtype=np.int64))
    assert d == want and (random.random(), np.random.uniform(0, 1)) == after
    with pytest.raises(ValueError, match="bounding boxes"):
        tf.draw(3, 48, 48)


def test_from_ids_maps_the_references_list():
    tf = TrainTransform2D.from_ids(2, [1, 3, 4, 6, 7, 8, 9, 10])
    assert (tf.normalize, tf.erase, tf.zoom, tf.degrees, tf.flip, tf.gamma, tf.noise) == \
        ("mr", (64, 64), (0.8, 1.2), tuple(REFERENCE_DEGREES), "hv", (0.8, 1.2), True)
    tf = TrainTransform2D.from_ids(2, [1, 6, 7, 10])                      # config.py's default
    assert (tf.normalize, tf.erase, tf.zoom, tf.degrees, tf.flip, tf.gamma, tf.noise) == \
        ("mr", None, None, tuple(REFERENCE_DEGREES), "hv", None, False)
    tf = TrainTransform2D.from_ids(2, [1, 3, 4, 6, 7, 8, 9, 10], train=False)   # trainer.py:173-176
    assert (tf.normalize, tf.erase, tf.zoom, tf.degrees, tf.flip, tf.gamma, tf.noise) == \
        ("mr", None, None, (), "", None, False)
    tf = TrainTransform2D.from_ids(2, [4, 10])
    assert (tf.normalize, tf.zoom, tf.degrees, tf.flip) == (None, (0.8, 1.2), (), "")


@pytest.mark.parametrize("bad,name", [(2, "CropResize"), (5, "RandomDistort2D"), (11, "Trunc_and_Normalize")])
def test_from_ids_refuses_by_name(bad, name):
    with pytest.raises(ValueError, match=name):
        TrainTransform2D.from_ids(2, sorted([1, 6, 7, 10, bad]))
    with pytest.raises(ValueError, match=name):
        TrainTransform2D.from_ids(2, sorted([1, 10, bad]), train=False)


def test_from_ids_and_the_constructor_refuse_what_they_cannot_run():
    with pytest.raises(ValueError, match="not in the reference's list"):
        TrainTransform2D.from_ids(2, [1, 12])
    with pytest.raises(ValueError, match="ascending"):
        TrainTransform2D.from_ids(2, [1, 7, 6, 10])
    with pytest.raises(ValueError, match="To_Tensor"):
        TrainTransform2D.from_ids(2, [1, 6, 7])
    with pytest.raises(ValueError, match="noise needs normalize='mr'"):
        TrainTransform2D.from_ids(2, [9, 10])
    with pytest.raises(ValueError, match="noise needs normalize='mr'"):
        TrainTransform2D(2, normalize=None, noise=True)
    with pytest.raises(ValueError, match="zoom must be"):
        TrainTransform2D(2, zoom=0.8)


# --------------------------------------------------------------------------------------- the restatement of section 3
def test_gamma_restatement():
    x = np.array([0.0, 1.0, 0.25, 0.5, -0.5], dtype=np.float32)
    got = zr.gamma_ref(x, 0.5)
    assert got.dtype == np.float32 and got.tolist() == [0.0, 1.0, 0.5, np.float32(np.sqrt(np.float64(0.5))), 0.0]
    assert zr.gamma_ref(x, 1.0).tobytes() == x.tobytes()                 # gamma 1: the bits, the negative included
    assert zr.gamma_ref(x, 1.0 + 1e-12).tobytes() == x.tobytes()         # rounds to 1.0f
    g = 0.8123456789
    assert zr.gamma_ref(x, g)[2] == np.float32(np.power(np.float64(0.25), np.float64(np.float32(g))))


def test_philox_matches_the_published_vectors():
    """Random123's known-answer tests for philox4x32-10"""
    def run(counter, key):
        return [int(v[0]) for v in zr.philox4x32([np.array([c], dtype=np.uint64) for c in counter], key)]
    assert run((0, 0, 0, 0), (0, 0)) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert run((0xffffffff,) * 4, (0xffffffff,) * 2) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    assert run((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0)) == \
        [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]


def test_normal_restatement_is_standard_normal_and_keyed():
    n = 1 << 15
    z = zr.normal_ref(7, 0, n)
    from math import erf, log, sqrt
    cdf = np.array([0.5 * (1.0 + erf(v / sqrt(2.0))) for v in np.sort(z)])
    d = max(np.abs(cdf - np.arange(1, n + 1) / n).max(), np.abs(cdf - np.arange(n) / n).max())
    assert d < sqrt(log(2 / 1e-9) / (2 * n))                             # the DKW bound at alpha = 1e-9
    assert not np.array_equal(z, zr.normal_ref(8, 0, n)) and not np.array_equal(z, zr.normal_ref(7, 1, n))
    assert np.array_equal(z[:100], zr.normal_ref(7, 0, 100))             # a function of the index, not of the count


# ------------------------------------------------------------------------------------------- (d) the entries, no CPU path
def test_the_symbols_are_exported_with_the_declared_signatures():
    hdr = " ".join(open(os.path.join(ROOT, "include", "hdf.h")).read().split())
    decls = (
        "int64_t hdf_label_bbox_workspace_bytes(int batch);",
        "int hdf_label_bbox_2d(const uint8_t* labels, int batch, int H, int W, int32_t* bbox, void* workspace, "
        "int64_t workspace_bytes, hdf_stream stream);",
        "int hdf_zoom_2d(const float* image, const uint8_t* labels, int batch, int channels, int H, int W, "
        "const int32_t* keep, const int32_t* canvas, float* image_out, uint8_t* labels_out, hdf_stream stream);",
        "int hdf_intensity_2d(float* image, int batch, int channels, int H, int W, const double* gamma, "
        "const uint8_t* noise, uint64_t seed, float low_clip, hdf_stream stream);")
    for decl in decls:
        assert decl in hdr, decl
    lib = _lib.lib()
    vp, i, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    want = {"hdf_label_bbox_workspace_bytes": (i64, [i]),
            "hdf_label_bbox_2d": (i, [vp, i, i, i, vp, vp, i64, vp]),
            "hdf_zoom_2d": (i, [vp, vp, i, i, i, i, vp, vp, vp, vp, vp]),
            "hdf_intensity_2d": (i, [vp, i, i, i, i, ctypes.POINTER(ctypes.c_double), vp, ctypes.c_uint64,
                                     ctypes.c_float, vp])}
    for name, (res, args) in want.items():
        assert name in _lib.EXPORTS
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    assert lib.hdf_label_bbox_workspace_bytes(24) > 0
    import hdf_rt
    for name in ("erase2d_keep", "gamma2d", "intensity_2d_", "label_bbox_2d", "noise2d_flag", "zoom2d_canvas", "zoom_2d"):
        assert name in dir(hdf_rt) and getattr(hdf_rt, name) is getattr(hdf_rt.augment, name)


def test_entries_refuse_null_arrays():
    """the refusals that can be provoked without a device: null pointers are checked before anything else, so nothing can
    launch.  Every other refusal is exercised with real device buffers in tests/test_gpu_transforms2d.py."""
    lib = _lib.lib()
    four = np.zeros(4, dtype=np.int32)
    rc = lib.hdf_zoom_2d(None, None, 1, 2, 4, 5, None, four.ctypes.data, None, None, None)
    assert rc == 1 and lib.hdf_last_error().startswith(b"zoom_2d: null keep"), (rc, lib.hdf_last_error())
    rc = lib.hdf_zoom_2d(None, None, 1, 2, 4, 5, four.ctypes.data, None, None, None, None)
    assert rc == 1 and lib.hdf_last_error().startswith(b"zoom_2d: null canvas"), (rc, lib.hdf_last_error())
    rc = lib.hdf_zoom_2d(None, None, 1, 2, 4, 5, four.ctypes.data, four.ctypes.data, None, None, None)
    assert rc == 1 and lib.hdf_last_error().startswith(b"zoom_2d: no output"), (rc, lib.hdf_last_error())
    rc = lib.hdf_label_bbox_2d(None, 1, 4, 5, None, None, 0, None)
    assert rc == 1 and lib.hdf_last_error().startswith(b"label_bbox_2d: null argument"), (rc, lib.hdf_last_error())
    one = np.ones(1, dtype=np.float64)
    rc = lib.hdf_intensity_2d(None, 1, 2, 4, 5, one.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), None, 0, 0.0, None)
    assert rc == 1 and lib.hdf_last_error().startswith(b"intensity_2d: null argument"), (rc, lib.hdf_last_error())


def test_the_new_calls_fail_loudly_without_a_gpu():
    image, labels = torch.zeros(2, 2, 5, 6), torch.zeros(2, 5, 6, dtype=torch.uint8)
    with pytest.raises(_lib.HdfError, match="no CPU path"):
        label_bbox_2d(labels)
    with pytest.raises(_lib.HdfError, match="no CPU path"):
        zoom_2d(image, labels, [(0, 5, 0, 6)] * 2, [(6, 5, 0, 0)] * 2)
    with pytest.raises(_lib.HdfError, match="no CPU path"):
        intensity_2d_(image, [1.0, 1.0], [0, 0])
    with pytest.raises(_lib.HdfError, match="no CPU path"):
        TrainTransform2D.from_ids(2, [1, 3, 4, 6, 7, 8, 9, 10])(image, labels)
