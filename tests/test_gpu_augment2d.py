"""hdf_augment_2d (include/hdf.h, csrc/augment.hip) called directly through ctypes and held BIT FOR BIT to
tests/augment2d_ref.py, the numpy restatement of PIL's rotate (itself held to PIL by tests/test_augment2d_ref_cpu.py):
image elements are compared as uint32, labels and one-hot as bytes; there is no tolerance anywhere in this file.  Every
call writes into one sentinel-filled block with guard bands between and around the three outputs: an output not asked
for, and every guard, must come back untouched, and the sources must be unchanged afterwards.
  exact, B = 3, C = 2, n_cls = 4 (labels 200 and 255 present), 37x43 and 43x37: angles (-15, 0, 10) with flips (1, 0, 2)
      in one batch; all seven reference angles x three flips at B = 1; outputs asked for singly and together
  closed forms: the identity matrix = the input and its hdf_onehot_from_labels; a flip alone = torch.flip; 180 degrees =
      the double flip
  more samples than one parameter chunk: B = 33 at 5x7, a distinct angle per sample
  past the grid cap: B = 2 at 520x517, 537,680 pixels against 2048 x 256 threads, so every thread's loop runs 1 or 2 trips
  degenerate 1x1, 1x9, 9x1, 2x2
  errors (aliased source / output, n_cls = 9, label output without labels, no output, a null or NaN matrix, a matrix past
      PIL's +-32768 corner check, flips[i] = 3, sizes out of range) return non-zero with a message and launch nothing;
      augment_2d raises ValueError for an output tensor of the wrong device, dtype, shape or stride before the call
  TrainTransform2D (B = 35, C = 2: 70 planes, more than one normalisation group and more than one parameter chunk): bit
      for bit clone -> per-plane mr_normalize_ -> augment_2d under the same draws; the validation form; a batch of 24 at
      2x64x64 straight into models.HDenseFormer_2D and the loss."""
import ctypes as C
import functools
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import augment2d_ref as ar  # noqa: E402
from hdf_rt._lib import check, lib, ptr  # noqa: E402
from hip_util import DEV, st  # noqa: E402

SENTINEL = 0xA5
GUARD = 1024          # bytes, a multiple of every element size
CHUNK = 32            # samples per launch (csrc/augment.h AUG2D_CHUNK)
GRID_THREADS = 2048 * 256


@functools.lru_cache(maxsize=None)
def _inputs(batch, channels, shape, seed=1):
    image = np.stack([ar.image_of(shape, channels, seed + 10 * b) for b in range(batch)])
    image[:, -1] *= 100.0
    labels = np.stack([ar.labels_of(shape, seed + 10 * b) for b in range(batch)])
    image.setflags(write=False), labels.setflags(write=False)
    return image, labels


def _matrices(angles, shape):
    return np.array([ar.matrix_of(a, shape[1], shape[0]) for a in angles], dtype=np.float64)


@functools.lru_cache(maxsize=None)
def _reference(batch, channels, shape, n_cls, angles, flips, seed=1):
    image, labels = _inputs(batch, channels, shape, seed)
    ref = ar.augment2d_batch_ref(image, labels, n_cls, _matrices(angles, shape), flips)
    for v in ref.values():
        v.setflags(write=False)
    return ref


def _call(image, labels, batch, channels, n_cls, shape, matrices, flips, io, lo, oo):
    mats = None if matrices is None else np.ascontiguousarray(matrices, dtype=np.float64)
    codes = None if flips is None else np.ascontiguousarray(flips, dtype=np.uint8)
    return lib().hdf_augment_2d(ptr(image), ptr(labels), batch, channels, n_cls, shape[0], shape[1],
                                None if mats is None else mats.ctypes.data_as(C.POINTER(C.c_double)),
                                None if codes is None else codes.ctypes.data, ptr(io), ptr(lo), ptr(oo), st())


def _run(image, labels, n_cls, matrices, flips, want=("image", "labels", "onehot")):
    """one call on host arrays [B, C, H, W] / [B, H, W]; returns {name: numpy array} of the outputs asked for, after
    checking that everything else in the output block still holds the sentinel and that the sources are unchanged"""
    batch, channels, shape = image.shape[0], image.shape[1], tuple(image.shape[2:])
    pix = batch * shape[0] * shape[1]
    sizes = {"image": 4 * channels * pix, "labels": pix, "onehot": 4 * n_cls * pix}
    start, pos = {}, GUARD
    for k in ("image", "labels", "onehot"):
        start[k] = pos
        pos += -(-sizes[k] // GUARD) * GUARD + GUARD
    block = torch.full((pos,), SENTINEL, dtype=torch.uint8, device=DEV)
    view = {k: block[start[k]: start[k] + sizes[k]] for k in sizes}
    di, dl = torch.tensor(image).to(DEV), torch.tensor(labels).to(DEV)
    check(_call(di, dl, batch, channels, n_cls, shape, matrices, flips, *[view[k] if k in want else None for k in sizes]),
          "hdf_augment_2d")
    host = block.cpu().numpy()
    assert torch.equal(di.cpu(), torch.tensor(image)) and torch.equal(dl.cpu(), torch.tensor(labels))
    written = np.zeros(pos, dtype=bool)
    out = {}
    for k in want:
        written[start[k]: start[k] + sizes[k]] = True
        raw = host[start[k]: start[k] + sizes[k]]
        out[k] = (raw.reshape((batch,) + shape) if k == "labels"
                  else raw.view(np.float32).reshape((batch, channels if k == "image" else n_cls) + shape))
    assert (host[~written] == SENTINEL).all(), "bytes outside the outputs asked for were written"
    return out


def _check_against(out, ref, what):
    for k in out:
        ar.check_exact(out[k], ref[k], "%s %s" % (what, k))


# ------------------------------------------------------------------------------------------------------------- exact
BATCH_ANGLES, BATCH_FLIPS = (-15, 0, 10), (1, 0, 2)


@pytest.mark.parametrize("shape", [(37, 43), (43, 37)], ids=["37x43", "43x37"])
def test_batch_with_different_angles_and_flips_is_exact(shape):
    image, labels = _inputs(3, 2, shape)
    assert (labels == 200).any() and (labels == 255).any() and (image < 0).any()
    ref = _reference(3, 2, shape, 4, BATCH_ANGLES, BATCH_FLIPS)
    assert (ref["image"] == 0).mean() > 0.005 and (ref["labels"] >= 200).any()   # corners left the plane; raw bytes moved
    out = _run(image, labels, 4, _matrices(BATCH_ANGLES, shape), BATCH_FLIPS)
    _check_against(out, ref, "batch %dx%d" % shape)


@pytest.mark.parametrize("flip", [0, 1, 2], ids=["noflip", "w", "h"])
def test_every_reference_angle_is_exact(flip):
    shape = (37, 43)
    image, labels = _inputs(1, 2, shape)
    for angle in ar.REFERENCE_DEGREES:
        ref = _reference(1, 2, shape, 4, (angle,), (flip,))
        out = _run(image, labels, 4, _matrices((angle,), shape), (flip,))
        _check_against(out, ref, "%d degrees flip %d" % (angle, flip))


@pytest.mark.parametrize("want", [("image",), ("labels",), ("onehot",), ("image", "onehot"), ("labels", "onehot")],
                         ids="+".join)
def test_outputs_asked_for_singly_leave_the_others_untouched(want):
    shape = (43, 37)
    image, labels = _inputs(3, 2, shape)
    ref = _reference(3, 2, shape, 4, BATCH_ANGLES, BATCH_FLIPS)
    out = _run(image, labels, 4, _matrices(BATCH_ANGLES, shape), BATCH_FLIPS, want)
    assert set(out) == set(want)
    _check_against(out, ref, "+".join(want))


def test_image_only_call_takes_null_labels_and_label_only_call_a_null_image():
    shape = (37, 43)
    image, labels = _inputs(3, 2, shape)
    ref = _reference(3, 2, shape, 4, BATCH_ANGLES, BATCH_FLIPS)
    mats = _matrices(BATCH_ANGLES, shape)
    di, dl = torch.tensor(image).to(DEV), torch.tensor(labels).to(DEV)
    io = torch.empty_like(di)
    check(_call(di, None, 3, 2, 4, shape, mats, BATCH_FLIPS, io, None, None), "hdf_augment_2d")
    ar.check_exact(io.cpu().numpy(), ref["image"], "image")
    lo = torch.empty_like(dl)
    check(_call(None, dl, 3, 0, 4, shape, mats, BATCH_FLIPS, None, lo, None), "hdf_augment_2d")
    ar.check_exact(lo.cpu().numpy(), ref["labels"], "labels")


# ------------------------------------------------------------------------------------------------------ closed forms
def test_identity_returns_the_input_and_its_onehot():
    shape = (37, 43)
    image, labels = _inputs(3, 2, shape)
    out = _run(image, labels, 4, [ar.IDENTITY] * 3, (0, 0, 0))
    ar.check_exact(out["image"], image, "image")
    ar.check_exact(out["labels"], labels, "labels")                  # the raw byte, 200 and 255 included
    dl = torch.tensor(labels).to(DEV)
    oh = torch.empty((3, 4) + shape, dtype=torch.float32, device=DEV)
    check(lib().hdf_onehot_from_labels(ptr(dl), ptr(oh), 3, 4, shape[0] * shape[1], st()), "hdf_onehot_from_labels")
    ar.check_exact(out["onehot"], oh.cpu().numpy(), "one-hot")
    # and rotate_matrix(0) is that identity, so PIL's short cut for 0 degrees needs no special case
    ar.check_exact(_run(image, labels, 4, _matrices((0, 0, 0), shape), (0, 0, 0))["image"], image, "0 degrees")


def test_a_flip_alone_is_torch_flip():
    shape = (37, 43)
    image, labels = _inputs(3, 2, shape)
    flips = (1, 2, 0)
    out = _run(image, labels, 4, [ar.IDENTITY] * 3, flips)
    for b, dims in enumerate(([-1], [-2], [])):
        want_i = torch.flip(torch.tensor(image[b]), dims).numpy()
        want_l = torch.flip(torch.tensor(labels[b]), dims).numpy()
        ar.check_exact(out["image"][b], want_i, "image %d" % b)
        ar.check_exact(out["labels"][b], want_l, "labels %d" % b)
        ar.check_exact(out["onehot"][b], ar.onehot_of(want_l, 4), "one-hot %d" % b)


@pytest.mark.parametrize("shape", [(37, 43), (24, 24)], ids=["37x43", "24x24"])
def test_180_degrees_is_the_double_flip(shape):
    image, labels = _inputs(2, 2, shape)
    out = _run(image, labels, 4, _matrices((180, 180), shape), (0, 0))
    ar.check_exact(out["image"], torch.flip(torch.tensor(image), [-2, -1]).numpy(), "image")
    want_l = torch.flip(torch.tensor(labels), [-2, -1]).numpy()
    ar.check_exact(out["labels"], want_l, "labels")
    ar.check_exact(out["onehot"], np.stack([ar.onehot_of(l, 4) for l in want_l]), "one-hot")


# ------------------------------------------------------------------------------------------- chunks, grid cap, shapes
def test_more_samples_than_one_parameter_chunk():
    shape, batch = (5, 7), CHUNK + 1
    angles = tuple(-16.5 + b for b in range(batch))                  # a distinct angle per sample
    flips = tuple(b % 3 for b in range(batch))
    image, labels = _inputs(batch, 2, shape)
    ref = _reference(batch, 2, shape, 4, angles, flips)
    assert len({r.tobytes() for r in _matrices(angles, shape)}) == batch
    out = _run(image, labels, 4, _matrices(angles, shape), flips)
    _check_against(out, ref, "%d samples" % batch)
    for b in (CHUNK - 1, CHUNK):                                     # the last of chunk 0 and the first of chunk 1 differ
        assert not np.array_equal(ref["image"][b], ref["image"][b - 1])


def test_past_the_grid_cap():
    shape, batch = (520, 517), 2
    assert GRID_THREADS < batch * shape[0] * shape[1] < 2 * GRID_THREADS   # every thread takes 1 or 2 trips
    angles, flips = (15, -10), (2, 1)
    image, labels = _inputs(batch, 2, shape)
    ref = _reference(batch, 2, shape, 3, angles, flips)
    out = _run(image, labels, 3, _matrices(angles, shape), flips)
    _check_against(out, ref, "520x517")


@pytest.mark.parametrize("shape", [(1, 1), (1, 9), (9, 1), (2, 2)], ids=lambda s: "%dx%d" % s)
def test_degenerate_shapes(shape):
    angles, flips = (0, 5, 90, 181, -15), (0, 1, 2, 1, 2)
    image, labels = _inputs(5, 2, shape)
    ref = _reference(5, 2, shape, 3, angles, flips)
    out = _run(image, labels, 3, _matrices(angles, shape), flips)
    _check_against(out, ref, "%dx%d" % shape)


# ------------------------------------------------------------------------------------------------------------ errors
def test_bad_arguments_are_refused_before_any_launch():
    shape = (37, 43)
    image, labels = _inputs(3, 2, shape)
    pix = labels.size
    mats = _matrices(BATCH_ANGLES, shape)
    di, dl = torch.tensor(image).to(DEV), torch.tensor(labels).to(DEV)
    io = torch.full((3, 2) + shape, -3.0, device=DEV)
    lo = torch.full((3,) + shape, 77, dtype=torch.uint8, device=DEV)
    oo = torch.full((3, 9) + shape, -3.0, device=DEV)
    two = torch.from_numpy(np.concatenate([image.reshape(-1), image.reshape(-1)])).to(DEV)
    nan = mats.copy()
    nan[1, 4] = np.nan
    inf = mats.copy()
    inf[2, 2] = np.inf
    far = mats.copy()
    far[1, 2] = 32768.0 - 20.0                                       # corner (W, 0) lands past 32768, corner (0, 0) does not
    steep = mats.copy()
    steep[0, 3] = -900.0                                             # |d W| = 38700
    cases = {
        "image_out is the image": dict(io=di),
        "labels_out is the labels": dict(lo=dl),
        "image_out overlaps the image's tail": dict(image=two[:2 * pix], io=two[2 * pix - 1: 4 * pix - 1]),
        "onehot_out overlaps the image": dict(image=two[:2 * pix], oo=two[pix: 5 * pix]),
        "nine classes": dict(n_cls=9),
        "one class": dict(n_cls=1),
        "labels_out without labels": dict(labels=None, oo=None),
        "onehot_out without labels": dict(labels=None, lo=None),
        "no output": dict(io=None, lo=None, oo=None),
        "an image output without an image": dict(image=None),
        "null matrices": dict(mats=None),
        "null flips": dict(flips=None),
        "NaN matrix": dict(mats=nan),
        "infinite matrix": dict(mats=inf),
        "matrix past the corner check (offset)": dict(mats=far),
        "matrix past the corner check (slope)": dict(mats=steep),
        "flip code 3": dict(flips=(0, 3, 1)),
        "no sample": dict(batch=0),
        "zero height": dict(shape=(0, 43)),
        "negative width": dict(shape=(37, -1)),
        "too wide": dict(shape=(1, 16385)),
        "65 channels": dict(channels=65),
        "no channel": dict(channels=0),
    }
    for what, over in cases.items():
        a = dict(image=di, labels=dl, batch=3, channels=2, n_cls=4, shape=shape, mats=mats, flips=BATCH_FLIPS, io=io,
                 lo=lo, oo=oo)
        a.update(over)
        rc = _call(a["image"], a["labels"], a["batch"], a["channels"], a["n_cls"], a["shape"], a["mats"], a["flips"],
                   a["io"], a["lo"], a["oo"])
        assert rc != 0 and lib().hdf_last_error().startswith(b"augment_2d:"), (what, rc, lib().hdf_last_error())
        if what == "NaN matrix":
            assert lib().hdf_last_error().startswith(b"augment_2d: matrices[1][4]")
        if what.startswith("matrix past"):
            assert b"32768" in lib().hdf_last_error()
        if what == "flip code 3":
            assert lib().hdf_last_error().startswith(b"augment_2d: flips[1]=3")
    torch.cuda.synchronize()
    assert torch.equal(di.cpu(), torch.tensor(image)) and torch.equal(dl.cpu(), torch.tensor(labels))
    assert bool((io == -3.0).all()) and bool((lo == 77).all()) and bool((oo == -3.0).all())
    assert torch.equal(two[:2 * pix].cpu().reshape(image.shape), torch.tensor(image))
    # the largest offset the corner check lets through is accepted (and maps every pixel outside: zeros)
    edge = np.array([[1.0, 0.0, 32767.0 - 43.0, 0.0, 1.0, 0.0]] * 3)
    check(_call(di, dl, 3, 2, 4, shape, edge, (0, 0, 0), io, lo, oo[:, :4].contiguous()), "hdf_augment_2d")
    assert bool((io == 0).all()) and bool((lo == 0).all())


def test_augment_2d_refuses_a_wrong_argument_before_the_call():
    """every tensor the kernel writes through is checked for device, dtype, shape and contiguity in Python: the C entry
    sees only addresses and would write through whatever it is given"""
    from hdf_rt import augment_2d
    shape = (37, 43)
    h, w = shape
    image, labels = _inputs(3, 2, shape)
    mats = _matrices(BATCH_ANGLES, shape)
    di, dl = torch.tensor(image).to(DEV), torch.tensor(labels).to(DEV)
    good = {"out_image": torch.full((3, 2, h, w), -3.0, device=DEV),
            "out_onehot": torch.full((3, 4, h, w), -3.0, device=DEV),
            "out_labels": torch.full((3, h, w), 77, dtype=torch.uint8, device=DEV)}
    wide = torch.full((3, h, 2 * w), 77, dtype=torch.uint8, device=DEV)
    bad = {
        "out_labels": {"int64": torch.full((3, h, w), 77, dtype=torch.int64, device=DEV),
                       "too small": torch.full((3, h, w - 1), 77, dtype=torch.uint8, device=DEV),
                       "one sample short": torch.full((2, h, w), 77, dtype=torch.uint8, device=DEV),
                       "flat": torch.full((3 * h * w,), 77, dtype=torch.uint8, device=DEV),
                       "strided": wide[:, :, ::2],
                       "host": torch.full((3, h, w), 77, dtype=torch.uint8),
                       "not a tensor": np.zeros((3, h, w), dtype=np.uint8)},
        "out_image": {"half": torch.full((3, 2, h, w), -3.0, dtype=torch.float16, device=DEV),
                      "one channel short": torch.full((3, 1, h, w), -3.0, device=DEV),
                      "strided": torch.full((3, 2, h, 2 * w), -3.0, device=DEV)[..., ::2]},
        "out_onehot": {"three classes": torch.full((3, 3, h, w), -3.0, device=DEV),
                       "host": torch.full((3, 4, h, w), -3.0)},
    }
    for arg, cases in bad.items():
        for what, t in cases.items():
            with pytest.raises(ValueError, match=arg):
                augment_2d(di, dl, 4, mats, BATCH_FLIPS, **{**good, arg: t})
            if torch.is_tensor(t):
                assert bool((t == (77 if t.dtype in (torch.uint8, torch.int64) else -3.0)).all()), (arg, what)
    with pytest.raises(ValueError, match="a label output needs labels"):
        augment_2d(di, None, 4, mats, BATCH_FLIPS, out_labels=good["out_labels"])
    with pytest.raises(ValueError, match="labels must be"):
        augment_2d(di, dl.long(), 4, mats, BATCH_FLIPS)
    with pytest.raises(ValueError, match="labels must be"):
        augment_2d(di, dl[:2], 4, mats, BATCH_FLIPS)
    with pytest.raises(ValueError, match="matrices must be"):
        augment_2d(di, dl, 4, mats[:2], BATCH_FLIPS)
    with pytest.raises(ValueError, match="flips must be"):
        augment_2d(di, dl, 4, mats, (0, 1))
    with pytest.raises(ValueError, match="flips must be"):
        augment_2d(di, dl, 4, mats, (0, 3, 1))
    with pytest.raises(ValueError, match="image must be"):
        augment_2d(di[0], dl, 4, mats, BATCH_FLIPS)
    torch.cuda.synchronize()
    assert bool((wide == 77).all())
    assert bool((good["out_image"] == -3.0).all()) and bool((good["out_onehot"] == -3.0).all())
    assert bool((good["out_labels"] == 77).all())
    r_i, r_o = augment_2d(di, dl, 4, mats, BATCH_FLIPS, **good)                  # and the good set is accepted
    assert r_i.data_ptr() == good["out_image"].data_ptr() and r_o.data_ptr() == good["out_onehot"].data_ptr()
    ref = _reference(3, 2, shape, 4, BATCH_ANGLES, BATCH_FLIPS)
    _check_against({"image": r_i.cpu().numpy(), "onehot": r_o.cpu().numpy(), "labels": good["out_labels"].cpu().numpy()},
                   ref, "augment_2d")
    n_i, n_o = augment_2d(di, None, 4, mats, BATCH_FLIPS)                        # image only: no one-hot
    assert n_o is None
    ar.check_exact(n_i.cpu().numpy(), ref["image"], "image only")


# ------------------------------------------------------------------------------------------------ the Python chain
def _raw_batch(batch, shape):
    rng = np.random.RandomState(21)
    image = rng.standard_normal((batch, 2) + shape).astype(np.float32)
    image[:, 0] = image[:, 0] * 300.0 + 400.0                        # MR-like range, some negatives: the clamp bites
    image[batch // 2, 1] = 0.0                                       # a plane whose maximum is 0 is left alone
    labels = np.stack([ar.labels_of(shape, 21 + b) for b in range(batch)])
    return torch.tensor(image).to(DEV), torch.tensor(labels).to(DEV)


def test_train_transform_is_the_chain_of_its_parts_under_the_same_draws():
    from hdf_rt import TrainTransform2D, augment_2d, flip2d_code, rotate_degree, rotate_matrix
    from hdf_rt.inference import mr_normalize_
    shape, batch = (17, 29), CHUNK + 3                               # 70 planes: two normalisation groups, two chunks
    image, labels = _raw_batch(batch, shape)
    assert bool((image < 0).any())
    keep_i, keep_l = image.clone(), labels.clone()
    tf = TrainTransform2D(3)
    for seed in (0, 1):
        random.seed(seed), np.random.seed(seed)
        got_i, got_oh = tf(image, labels)
        assert torch.equal(image, keep_i) and torch.equal(labels, keep_l)        # the arguments are left alone
        random.seed(seed), np.random.seed(seed)
        norm = image.clone()
        for b in range(batch):
            for c in range(2):
                mr_normalize_(norm[b, c][None])                                  # per plane, one at a time
        assert float(norm.min()) == 0.0 and float(norm[:, 0].amax()) == 1.0
        mats, codes = [], []
        for _ in range(batch):                                                   # the degree first, the flip second
            mats.append(rotate_matrix(rotate_degree(), shape[1], shape[0]))
            codes.append(flip2d_code("hv"))
        assert len(set(mats)) > 3 and set(codes) == {0, 1, 2}
        want_i, want_oh = augment_2d(norm, labels, 3, mats, codes)
        assert got_i.shape == (batch, 2) + shape and got_oh.shape == (batch, 3) + shape
        assert torch.equal(got_i, want_i) and torch.equal(got_oh, want_oh)
        # and the parts are the restatement's: the rotation of the normalised batch
        ref = ar.augment2d_batch_ref(norm.cpu().numpy(), labels.cpu().numpy(), 3, mats, codes)
        _check_against({"image": got_i.cpu().numpy(), "onehot": got_oh.cpu().numpy()}, ref, "TrainTransform2D")


def test_validation_form_is_normalise_and_onehot():
    from hdf_rt import TrainTransform2D
    from hdf_rt.inference import mr_normalize_, onehot_from_labels
    shape, batch = (17, 29), 5
    image, labels = _raw_batch(batch, shape)
    keep_i = image.clone()
    random.seed(4), np.random.seed(4)
    state, pstate = np.random.get_state()[1].copy(), random.getstate()
    got_i, got_oh = TrainTransform2D(3, degrees=(), flip="")(image, labels)
    assert np.array_equal(np.random.get_state()[1], state) and random.getstate() == pstate   # no augmentation draw
    assert torch.equal(image, keep_i)
    norm = image.clone()
    mr_normalize_(norm.view(batch * 2, 1, *shape))
    assert torch.equal(got_i, norm) and torch.equal(got_oh, onehot_from_labels(labels, 3))
    raw_i, _ = TrainTransform2D(3, normalize=None, degrees=(), flip="")(image, labels)
    assert torch.equal(raw_i, image) and raw_i.data_ptr() != image.data_ptr()


def test_a_batch_goes_straight_into_the_2d_model_and_the_loss():
    from hdf_rt import TrainTransform2D
    from loss.combine_loss import CEPlusDice, DeepSuperloss
    from models.HDenseFormer_2D import HDenseFormer_2D
    shape, batch, n_cls = (64, 64), 24, 3
    image, labels = _raw_batch(batch, shape)
    random.seed(2), np.random.seed(2)
    x, onehot = TrainTransform2D(n_cls)(image, labels)
    for t, ch in ((x, 2), (onehot, n_cls)):                          # what the model and the loss take as they are
        assert t.dtype == torch.float32 and t.is_contiguous() and t.device.type == "cuda"
        assert tuple(t.shape) == (batch, ch) + shape
    assert bool((onehot.sum(1) == 1).all())
    torch.manual_seed(0)
    net = HDenseFormer_2D(2, n_cls, 16, image_size=shape, transformer_depth=4).to(DEV).train()
    net.set_dropout_seed(3)
    outs = net(x)
    loss = DeepSuperloss(criterion=CEPlusDice(weight=None, ignore_index=0))(outs, onehot)
    loss.backward()
    torch.cuda.synchronize()
    assert tuple(outs[0].shape) == (batch, n_cls) + shape and bool(torch.isfinite(loss))
    grads = [p.grad for p in net.parameters() if p.grad is not None]
    assert grads and all(bool(torch.isfinite(g).all()) for g in grads)
