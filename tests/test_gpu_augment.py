"""hdf_augment_3d (include/hdf.h, csrc/augment.hip) called directly through ctypes and held to tests/augment_ref.py, the
fp64 restatement of the reference's RandomTranslationRotationZoom3D + RandomFlip3D + To_Tensor (itself held to scipy's
map_coordinates by tests/test_augment_ref_cpu.py).  Every call writes into one sentinel-filled block with guard bands
between and around the three outputs: an output not asked for, and every guard, must come back untouched.
  exact, 5x37x43, C = 3, n_cls = 4 (labels 200 and 255 present): identity = the input bit for bit and
      hdf_onehot_from_labels of the input; each flip = torch.flip; translation (1,-3,2) = a shifted copy with exact zeros
      outside; translation (0,0.5,0): every class sum in {0, 1/2, 1}, labels equal the restatement with NO exclusion
      (>=, last class wins, class beats background at 1/2)
  rounding, 5x37x43: matrices 'tr', 'trz' and a general 3-axis rotation with zoom (more than 10 % of the voxels with a
      corner outside the volume) x C in {1, 3} x n_cls in {2, 4} x {no flip, H, W}; image per element within
      2^-23 |ref| + 1e-11 vmax (augment_ref.check_image), labels exact outside the 1e-7 band around 0.5
      (augment_ref.check_labels: nothing excluded on these inputs); outputs asked for singly and together
  past the grid, 104x101x103, C = 2, n_cls = 3, 'tr': the launch is capped at 2048 x 256 threads, so every thread's
      grid-stride loop runs 2 or 3 trips
  degenerate 1x1x1 and 1x2x65; errors (aliased source / output, n_cls = 9, label output without labels, no output, a matrix
      that is null or not finite) return non-zero with a message and launch nothing; augment_3d raises ValueError for an
      output tensor of the wrong device, dtype, shape or stride before the call
  TrainTransform3D, source 20x45x50, patch 16x40x50, C = 2, n_cls = 3: bit-identical to slice -> pet_ct_normalize_ ->
      augment_3d under the same draws; the validation form equals slice + normalise + onehot_from_labels
Worst image error / bound ("ROUNDING augment ...", pytest -s) of the kernel's arithmetic compiled for the host and run
against the same references: tr 0.497, trz 0.498, rot3 0.496, tr 104x101x103 0.500, half-voxel 1x2x65 0.464, every exact
case 0.000; no voxel excluded from any label comparison.  An error of 0.5 x the bound is the one fp32 rounding."""
import ctypes as C
import functools
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import augment_ref as ar  # noqa: E402
from hdf_rt._lib import check, lib, ptr  # noqa: E402
from hip_util import DEV, st  # noqa: E402

SENTINEL = 0xA5
GUARD = 1024          # bytes, a multiple of every element size


@functools.lru_cache(maxsize=None)
def _inputs(shape, channels, n_cls, blocky=False):
    image, labels = ar.image_of(shape, channels, 1), ar.labels_of(shape, n_cls, 1, blocky)
    assert (image.min(axis=(1, 2, 3)) < 0).all() and (image.max(axis=(1, 2, 3)) > 0).all()
    assert (labels == 200).any() and (labels == 255).any()
    image.setflags(write=False), labels.setflags(write=False)
    return image, labels


@functools.lru_cache(maxsize=None)
def _reference(shape, channels, n_cls, name, flip_h, flip_w):
    image, labels = _inputs(shape, channels, n_cls)
    ref = ar.augment_ref(image, labels, n_cls, _matrix(name), flip_h, flip_w)
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


def _matrix(name):
    return {"identity": ar.IDENTITY, "half": ar.translation((0, 0.5, 0)), "shift": ar.translation((1, -3, 2)),
            **ar.MATRICES}[name]


def _call(image, labels, channels, n_cls, shape, affine, flip_h, flip_w, io, lo, oo):
    aff = np.ascontiguousarray(affine, dtype=np.float64)
    return lib().hdf_augment_3d(ptr(image), ptr(labels), channels, n_cls, shape[0], shape[1], shape[2],
                                aff.ctypes.data_as(C.POINTER(C.c_double)), int(flip_h), int(flip_w), ptr(io), ptr(lo),
                                ptr(oo), st())


def _run(image, labels, n_cls, affine, flip_h=False, flip_w=False, want=("image", "labels", "onehot")):
    """one call on host arrays; returns {name: numpy array} of the outputs asked for, after checking that everything
    else in the output block still holds the sentinel"""
    channels, shape = image.shape[0], tuple(image.shape[1:])
    vox = int(np.prod(shape))
    sizes = {"image": 4 * channels * vox, "labels": vox, "onehot": 4 * n_cls * vox}
    start, pos = {}, GUARD
    for k in ("image", "labels", "onehot"):
        start[k] = pos
        pos += -(-sizes[k] // GUARD) * GUARD + GUARD
    block = torch.full((pos,), SENTINEL, dtype=torch.uint8, device=DEV)
    view = {k: block[start[k]: start[k] + sizes[k]] for k in sizes}
    di, dl = torch.tensor(image).to(DEV), torch.tensor(labels).to(DEV)
    check(_call(di, dl, channels, n_cls, shape, affine, flip_h, flip_w, *[view[k] if k in want else None for k in sizes]),
          "hdf_augment_3d")
    host = block.cpu().numpy()
    assert torch.equal(di.cpu(), torch.tensor(image)) and torch.equal(dl.cpu(), torch.tensor(labels))
    written = np.zeros(pos, dtype=bool)
    out = {}
    for k in want:
        written[start[k]: start[k] + sizes[k]] = True
        raw = host[start[k]: start[k] + sizes[k]]
        out[k] = (raw.reshape(shape) if k == "labels"
                  else raw.view(np.float32).reshape((channels if k == "image" else n_cls,) + shape))
    assert (host[~written] == SENTINEL).all(), "bytes outside the outputs asked for were written"
    return out


def _check_against(out, ref, image, what, exact_labels=False):
    """every output present in `out` against the restatement; prints and returns the worst image error / bound.
    exact_labels: the class sums sit exactly on 0.5 by construction, so the class map must equal the restatement's"""
    worst = 0.0
    if "image" in out:
        for ch in range(image.shape[0]):
            worst = max(worst, ar.check_image(out["image"][ch], ref["image"][ch], np.abs(image[ch]).max(),
                                              "%s channel %d" % (what, ch)))
    share = 0.0

    def labels_ok(got, name):
        if exact_labels:
            ar.check_exact(got, ref["labels"], name)
            return 0.0
        return ar.check_labels(got, ref["sums"], name)

    if "labels" in out:
        share = labels_ok(out["labels"], what)
    if "onehot" in out:
        got = out["onehot"]
        assert set(np.unique(got)) <= {0.0, 1.0} and (got.sum(0) == 1).all()
        share = labels_ok(np.where(got[0] == 1, 0, got.argmax(0)).astype(np.uint8), what + " one-hot")
    if "labels" in out and "onehot" in out:
        ar.check_exact(out["onehot"], ar.onehot_of(out["labels"], out["onehot"].shape[0]), what + " one-hot of labels")
    print("ROUNDING augment %s image %.3f labels-excluded %.1e" % (what, worst, share), flush=True)
    return worst


# ------------------------------------------------------------------------------------------------------------- exact
def test_identity_returns_the_input_and_its_onehot():
    image, labels = _inputs(ar.SHAPE, 3, 4)
    out = _run(image, labels, 4, ar.IDENTITY)
    ar.check_exact(out["image"], image, "image")
    dl = torch.tensor(labels).to(DEV)
    oh = torch.empty((4,) + ar.SHAPE, dtype=torch.float32, device=DEV)
    check(lib().hdf_onehot_from_labels(ptr(dl), ptr(oh), 1, 4, labels.size, st()), "hdf_onehot_from_labels")
    ar.check_exact(out["onehot"], oh.cpu().numpy(), "one-hot")
    ar.check_exact(out["labels"], np.where(labels < 4, labels, 0).astype(np.uint8), "labels")


@pytest.mark.parametrize("flip_h,flip_w", [(True, False), (False, True), (True, True)], ids=["h", "w", "hw"])
def test_flip_with_the_identity_matrix_is_torch_flip(flip_h, flip_w):
    image, labels = _inputs(ar.SHAPE, 3, 4)
    out = _run(image, labels, 4, ar.IDENTITY, flip_h, flip_w)
    dims = [d for d, on in ((-2, flip_h), (-1, flip_w)) if on]
    ar.check_exact(out["image"], torch.flip(torch.tensor(image), dims).numpy(), "image")
    want = torch.flip(torch.from_numpy(np.where(labels < 4, labels, 0).astype(np.uint8)), dims).numpy()
    ar.check_exact(out["labels"], want, "labels")
    ar.check_exact(out["onehot"], ar.onehot_of(want, 4), "one-hot")


def test_integer_translation_is_a_shifted_copy_with_exact_zeros():
    image, labels = _inputs(ar.SHAPE, 3, 4)
    t = (1, -3, 2)
    out = _run(image, labels, 4, _matrix("shift"))
    d, h, w = ar.SHAPE
    want_i = np.zeros_like(image)
    want_l = np.zeros_like(labels)
    # out[p] = in[p + t] where p + t is inside
    want_i[:, :d - 1, 3:, :w - 2] = image[:, 1:, :h - 3, 2:]
    want_l[:d - 1, 3:, :w - 2] = np.where(labels < 4, labels, 0)[1:, :h - 3, 2:]
    assert t == (1, -3, 2)
    ar.check_exact(out["image"], want_i, "image")            # bytes: the zeros outside are +0.0
    ar.check_exact(out["labels"], want_l, "labels")
    ar.check_exact(out["onehot"], ar.onehot_of(want_l, 4), "one-hot")


def test_half_voxel_translation_decides_every_tie_like_the_reference():
    image, labels = _inputs(ar.SHAPE, 3, 4)
    ref = _reference(ar.SHAPE, 3, 4, "half", False, False)
    assert set(np.unique(ref["sums"])) <= {0.0, 0.5, 1.0} and int((ref["sums"] == 0.5).sum()) > 5000
    out = _run(image, labels, 4, _matrix("half"))
    ar.check_exact(out["labels"], ref["labels"], "labels")   # no exclusion
    ar.check_exact(out["onehot"], ref["onehot"], "one-hot")
    for ch in range(3):
        ar.check_image(out["image"][ch], ref["image"][ch], np.abs(image[ch]).max())


# ---------------------------------------------------------------------------------------------------------- rounding
@pytest.mark.parametrize("flip_h,flip_w", [(False, False), (True, False), (False, True)], ids=["noflip", "h", "w"])
@pytest.mark.parametrize("channels,n_cls", [(1, 2), (1, 4), (3, 2), (3, 4)])
@pytest.mark.parametrize("name", ["tr", "trz", "rot3"])
def test_warp_matches_the_restatement_to_one_rounding(name, channels, n_cls, flip_h, flip_w):
    image, labels = _inputs(ar.SHAPE, channels, n_cls)
    ref = _reference(ar.SHAPE, channels, n_cls, name, flip_h, flip_w)
    if name == "rot3":
        assert ref["outside"] > 0.10, ref["outside"]
    out = _run(image, labels, n_cls, _matrix(name), flip_h, flip_w)
    _check_against(out, ref, image, "%s C%d n%d %s" % (name, channels, n_cls, "h" if flip_h else "w" if flip_w else "-"))


@pytest.mark.parametrize("want", [("image",), ("labels",), ("onehot",), ("image", "onehot"), ("labels", "onehot")],
                         ids="+".join)
def test_outputs_asked_for_singly_leave_the_others_untouched(want):
    image, labels = _inputs(ar.SHAPE, 3, 4)
    ref = _reference(ar.SHAPE, 3, 4, "trz", True, False)
    out = _run(image, labels, 4, _matrix("trz"), True, False, want)
    assert set(out) == set(want)
    _check_against(out, ref, image, "trz " + "+".join(want))


def test_image_only_call_takes_null_labels():
    image, _ = _inputs(ar.SHAPE, 3, 4)
    ref = _reference(ar.SHAPE, 3, 4, "tr", False, False)
    di = torch.tensor(image).to(DEV)
    io = torch.empty_like(di)
    check(_call(di, None, 3, 4, ar.SHAPE, ar.TR, False, False, io, None, None), "hdf_augment_3d")
    for ch in range(3):
        ar.check_image(io[ch].cpu().numpy(), ref["image"][ch], np.abs(image[ch]).max())


def test_blocky_labels_match_the_restatement():
    image, _ = _inputs(ar.SHAPE, 3, 4)
    labels = ar.labels_of(ar.SHAPE, 4, 1, blocky=True)
    ref = ar.augment_ref(image, labels, 4, ar.TRZ, False, True)
    out = _run(image, labels, 4, ar.TRZ, False, True, ("labels", "onehot"))
    _check_against(out, ref, image, "trz blocky")


def test_past_the_grid_cap():
    shape = ar.BIG_SHAPE
    assert -(-int(np.prod(shape)) // 256) > 2 * 2048                 # every thread of the capped grid takes >= 2 trips
    image, labels = _inputs(shape, 2, 3)
    ref = _reference(shape, 2, 3, "tr", False, True)
    out = _run(image, labels, 3, ar.TR, False, True)
    _check_against(out, ref, image, "tr 104x101x103")


@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 2, 65)], ids=["1x1x1", "1x2x65"])
@pytest.mark.parametrize("name", ["identity", "half", "tr"])
def test_degenerate_shapes(shape, name):
    image = ar.image_of(shape, 2, 5)
    labels = np.random.RandomState(8).randint(1, 3, size=shape).astype(np.uint8)
    ref = ar.augment_ref(image, labels, 3, _matrix(name), False, True)
    out = _run(image, labels, 3, _matrix(name), False, True)
    if name == "identity":
        ar.check_exact(out["image"], ar.flip(image, False, True), "image")
    _check_against(out, ref, image, "%s %dx%dx%d" % ((name,) + shape), exact_labels=name != "tr")


# ------------------------------------------------------------------------------------------------------------ errors
def test_bad_arguments_are_refused_before_any_launch():
    image, labels = _inputs(ar.SHAPE, 3, 4)
    vox = labels.size
    di, dl = torch.tensor(image).to(DEV), torch.tensor(labels).to(DEV)
    io = torch.full((3,) + ar.SHAPE, -3.0, device=DEV)
    lo = torch.full(ar.SHAPE, 77, dtype=torch.uint8, device=DEV)
    oo = torch.full((9,) + ar.SHAPE, -3.0, device=DEV)
    two = torch.from_numpy(np.concatenate([image.reshape(-1), image.reshape(-1)])).to(DEV)
    cases = {
        "image_out is the image": (di, dl, 4, di, lo, oo),
        "labels_out is the labels": (di, dl, 4, io, dl, oo),
        "image_out overlaps the image's tail": (two[:3 * vox], dl, 4, two[3 * vox - 1: 6 * vox - 1], lo, oo),
        "onehot_out overlaps the image": (two[:3 * vox], dl, 4, io, lo, two[vox: 5 * vox]),
        "nine classes": (di, dl, 9, io, lo, oo),
        "one class": (di, dl, 1, io, lo, oo),
        "labels_out without labels": (di, None, 4, io, lo, None),
        "onehot_out without labels": (di, None, 4, io, None, oo),
        "no output": (di, dl, 4, None, None, None),
    }
    for what, (a, b, n_cls, x, y, z) in cases.items():
        rc = _call(a, b, 3, n_cls, ar.SHAPE, ar.TR, False, False, x, y, z)
        assert rc != 0 and lib().hdf_last_error().startswith(b"augment_3d:"), (what, rc, lib().hdf_last_error())
    nan = ar.TR.copy()
    nan[1, 3] = np.nan
    assert _call(di, dl, 3, 4, ar.SHAPE, nan, False, False, io, lo, oo) != 0
    assert lib().hdf_last_error().startswith(b"augment_3d: affine[7]")
    assert lib().hdf_augment_3d(ptr(di), ptr(dl), 3, 4, *ar.SHAPE, None, 0, 0, ptr(io), ptr(lo), ptr(oo), st()) != 0
    assert lib().hdf_last_error().startswith(b"augment_3d: null affine")
    for shape in [(0, 37, 43), (5, -1, 43)]:
        assert _call(di, dl, 3, 4, shape, ar.TR, False, False, io, lo, oo) != 0
    assert _call(di, dl, 65, 4, ar.SHAPE, ar.TR, False, False, io, lo, oo) != 0
    torch.cuda.synchronize()
    assert torch.equal(di.cpu(), torch.tensor(image)) and torch.equal(dl.cpu(), torch.tensor(labels))
    assert bool((io == -3.0).all()) and bool((lo == 77).all()) and bool((oo == -3.0).all())
    assert torch.equal(two[:3 * vox].cpu().reshape(image.shape), torch.tensor(image))


# ------------------------------------------------------------------------------------------------ the Python chain
def _raw_sample():
    rng = np.random.RandomState(21)
    image = rng.standard_normal((2, 20, 45, 50)).astype(np.float32)
    image[0] *= 700.0                                                # CT-like range: the clip of PETandCTNormalize bites
    labels = ar.labels_of((20, 45, 50), 3, 21, blocky=True)
    return torch.tensor(image).to(DEV), torch.tensor(labels).to(DEV)


def test_train_transform_is_the_chain_of_its_parts_under_the_same_draws():
    from hdf_rt import TrainTransform3D, augment_3d, crop_origin, flip_flags, trz_matrix
    from hdf_rt.inference import pet_ct_normalize_
    image, labels = _raw_sample()
    keep_i, keep_l = image.clone(), labels.clone()
    patch = (16, 40, 50)
    tf = TrainTransform3D(3, patch_size=patch, normalize="petct")
    for seed in (0, 1):
        random.seed(seed), np.random.seed(seed)
        got_i, got_oh = tf(image, labels)
        assert torch.equal(image, keep_i) and torch.equal(labels, keep_l)        # the arguments are left alone
        random.seed(seed), np.random.seed(seed)
        o = crop_origin(labels.shape, patch)
        assert o[2] == 0
        ci = image[:, o[0]:o[0] + 16, o[1]:o[1] + 40, :].contiguous()
        cl = labels[o[0]:o[0] + 16, o[1]:o[1] + 40, :].contiguous()
        pet_ct_normalize_(ci)
        aff, (fh, fw) = trz_matrix("tr"), flip_flags("hv")
        want_i, want_oh = augment_3d(ci, cl, 3, aff, fh, fw)
        assert got_i.shape == (2,) + patch and got_oh.shape == (3,) + patch
        assert torch.equal(got_i, want_i) and torch.equal(got_oh, want_oh)
        # and the parts are the restatement's: the warp of the normalised crop
        ref = ar.augment_ref(ci.cpu().numpy(), cl.cpu().numpy(), 3, aff, fh, fw)
        _check_against({"image": got_i.cpu().numpy(), "onehot": got_oh.cpu().numpy()}, ref, ci.cpu().numpy(),
                       "TrainTransform3D seed %d" % seed)


def test_batch_slices_are_written_in_place():
    from hdf_rt import augment_3d
    image, labels = _inputs(ar.SHAPE, 3, 4)
    di, dl = torch.tensor(image).to(DEV), torch.tensor(labels).to(DEV)
    bi = torch.full((2, 3) + ar.SHAPE, -3.0, device=DEV)
    bo = torch.full((2, 4) + ar.SHAPE, -3.0, device=DEV)
    lo = torch.full(ar.SHAPE, 77, dtype=torch.uint8, device=DEV)
    r_i, r_o = augment_3d(di, dl, 4, ar.TR, True, False, out_image=bi[1], out_onehot=bo[1], out_labels=lo)
    assert r_i.data_ptr() == bi[1].data_ptr() and r_o.data_ptr() == bo[1].data_ptr()
    assert bool((bi[0] == -3.0).all()) and bool((bo[0] == -3.0).all())
    ref = _reference(ar.SHAPE, 3, 4, "tr", True, False)
    _check_against({"image": bi[1].cpu().numpy(), "labels": lo.cpu().numpy(), "onehot": bo[1].cpu().numpy()}, ref, image,
                   "batch slice")


def test_augment_3d_refuses_a_wrong_output_tensor_before_the_call():
    """every tensor the kernel writes through is checked for device, dtype, shape and contiguity in Python: the C entry
    sees only addresses and would write V (or 4 C V, 4 n_cls V) bytes through whatever it is given"""
    from hdf_rt import augment_3d
    image, labels = _inputs(ar.SHAPE, 3, 4)
    d, h, w = ar.SHAPE
    di, dl = torch.tensor(image).to(DEV), torch.tensor(labels).to(DEV)
    good = {"out_image": torch.full((3, d, h, w), -3.0, device=DEV),
            "out_onehot": torch.full((4, d, h, w), -3.0, device=DEV),
            "out_labels": torch.full((d, h, w), 77, dtype=torch.uint8, device=DEV)}
    wide = torch.full((d, h, 2 * w), 77, dtype=torch.uint8, device=DEV)
    bad = {
        "out_labels": {"int64": torch.full((d, h, w), 77, dtype=torch.int64, device=DEV),
                       "too small": torch.full((d, h, w - 1), 77, dtype=torch.uint8, device=DEV),
                       "flat": torch.full((d * h * w,), 77, dtype=torch.uint8, device=DEV),
                       "strided": wide[:, :, ::2],
                       "host": torch.full((d, h, w), 77, dtype=torch.uint8),
                       "not a tensor": np.zeros((d, h, w), dtype=np.uint8)},
        "out_image": {"half": torch.full((3, d, h, w), -3.0, dtype=torch.float16, device=DEV),
                      "one channel short": torch.full((2, d, h, w), -3.0, device=DEV),
                      "strided": torch.full((3, d, h, 2 * w), -3.0, device=DEV)[..., ::2]},
        "out_onehot": {"three classes": torch.full((3, d, h, w), -3.0, device=DEV),
                       "host": torch.full((4, d, h, w), -3.0)},
    }
    for arg, cases in bad.items():
        for what, t in cases.items():
            with pytest.raises(ValueError, match=arg):
                augment_3d(di, dl, 4, ar.TR, **{**good, arg: t})
            if torch.is_tensor(t):
                assert bool((t == (77 if t.dtype in (torch.uint8, torch.int64) else -3.0)).all()), (arg, what)
    with pytest.raises(ValueError, match="a label output needs labels"):
        augment_3d(di, None, 4, ar.TR, out_labels=good["out_labels"])
    with pytest.raises(ValueError, match="labels must be"):
        augment_3d(di, dl.long(), 4, ar.TR)
    torch.cuda.synchronize()
    assert bool((wide == 77).all())
    assert bool((good["out_image"] == -3.0).all()) and bool((good["out_onehot"] == -3.0).all())
    assert bool((good["out_labels"] == 77).all())
    augment_3d(di, dl, 4, ar.TR, **good)                                         # and the good set is accepted
    assert not bool((good["out_labels"] == 77).any())


def test_validation_form_is_slice_normalise_onehot():
    from hdf_rt import TrainTransform3D, crop_origin
    from hdf_rt.inference import mr_normalize_, onehot_from_labels
    image, labels = _raw_sample()
    patch = (16, 40, 50)
    random.seed(4)
    state = np.random.get_state()[1].copy()
    got_i, got_oh = TrainTransform3D(3, patch_size=patch, normalize="mr", mode="", flip="")(image, labels)
    assert np.array_equal(np.random.get_state()[1], state)                       # no augmentation draw
    random.seed(4)
    o = crop_origin(labels.shape, patch)
    ci = image[:, o[0]:o[0] + 16, o[1]:o[1] + 40, :].contiguous()
    cl = labels[o[0]:o[0] + 16, o[1]:o[1] + 40, :].contiguous()
    assert torch.equal(got_i, mr_normalize_(ci)) and torch.equal(got_oh, onehot_from_labels(cl[None], 3)[0])
