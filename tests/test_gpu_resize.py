"""hdf_resize_3d and hdf_trunc_normalize (include/hdf.h, csrc/resize.hip) called directly through ctypes and held to
tests/resize_ref.py, the fp64 restatement of the resize of the reference's CropResize (itself held to live scipy by
tests/test_resize_ref_cpu.py).  Every call writes into one sentinel-filled block with guard bands between and around the
two outputs and the workspace: an output not asked for, every guard and both inputs must come back untouched.
  exact: equal shapes = the image bit for bit and where(l < n_cls, l, 0); a constant image 0.7 at 9x37x43 -> 6x24x48 =
      0.7f bit for bit; an all-background and an all-class-3 map = the restatement's map with NO exclusion in the
      interior; 2:3 along W puts class sums exactly on 0.5: `>=` and the last class winning, no exclusion
  rounding: the first six shapes of resize_ref.SHAPES x C in {1, 3} x n_cls in {2, 4}; image per element within
      2^-23 |ref| + 1e-11 vmax (augment_ref.check_image: one fp32 rounding), labels exact outside the 1e-7 band around
      0.5 (augment_ref.check_labels; blocky labels: nothing excluded); image-only, labels-only and joint calls
  past the grid, 104x101x103 -> 53x80x111, C = 2, n_cls = 3: a launch is capped at 2048 x 256 threads, so the grid-stride
      loop of the first pass (D, 53x101x103 outputs) runs more than one trip
  refusals: every bad argument returns non-zero with a "resize_3d:" / "trunc_normalize:" message and launches nothing;
      resize_3d raises ValueError for a tensor of the wrong device, dtype, shape or stride before the call
  trunc_normalize_: bit-identical to numpy's fp32 sequence on a CT-like volume, exactly lo and exactly hi included
  the chain, source 2x20x45x50, n_cls = 3: from_ids(3, [2,3,4,5,6], input_shape=(16,32,48)) is bit-identical to
      pet_ct_normalize_ -> crop_resize -> augment_3d under the same seeds, its train=False form to normalise ->
      crop_resize -> onehot_from_labels.  The model takes no depth below 32, so the step into models.HDenseFormer (16
      filters, depth 8) and DeepSuperloss(CEPlusDice) uses the same chain with input_shape=(32,32,48).
Worst image error / bound ("ROUNDING resize ...", pytest -s) on an MI355X: 9x37x43->6x24x48 0.496, 5x20x22->7x31x29 0.495,
8x37x43->1x24x48 0.494, 1x37x43->1x24x48 0.498, 16x3x8->2x3x1 0.373, 7x40x48->7x20x24 0.493, 104x101x103->53x80x111 0.500,
every exact case 0.000; no voxel excluded from any label comparison.  An error of 0.5 x the bound is the one fp32 rounding."""
import functools
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import augment_ref as ar  # noqa: E402
import resize_ref as rr  # noqa: E402
from hdf_rt._lib import check, lib, ptr  # noqa: E402
from hip_util import DEV, st  # noqa: E402

SENTINEL = 0xA5
GUARD = 1024          # bytes, a multiple of every element size
IDS = ["%dx%dx%d-%dx%dx%d" % (a + b) for a, b in rr.SHAPES[:6]]


@functools.lru_cache(maxsize=None)
def _inputs(shape, channels, n_cls):
    image, labels = ar.image_of(shape, channels, 1), ar.labels_of(shape, n_cls, 1, blocky=True)
    assert (labels == 200).any() and (labels == 255).any()
    image.setflags(write=False), labels.setflags(write=False)
    return image, labels


@functools.lru_cache(maxsize=None)
def _reference(src, dst, channels, n_cls):
    image, labels = _inputs(src, channels, n_cls)
    ref = rr.resize_ref(image, labels, n_cls, dst)
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


def _call(image, labels, channels, n_cls, src, dst, io, lo, ws, ws_bytes):
    return lib().hdf_resize_3d(ptr(image), ptr(labels), channels, n_cls, *src, *dst, ptr(io), ptr(lo), ptr(ws), ws_bytes,
                               st())


def _run(image, labels, n_cls, dst, want=("image", "labels")):
    """one call on host arrays (either may be None); returns {name: numpy array} of the outputs asked for, after checking
    that everything else in the block still holds the sentinel"""
    first = image if image is not None else labels
    src = tuple(first.shape[-3:])
    channels = image.shape[0] if image is not None else 0
    vout = int(np.prod(dst))
    need = int(lib().hdf_resize_workspace_bytes(*src, *dst))
    assert need >= 0
    sizes = {"image": 4 * max(channels, 1) * vout, "labels": vout, "ws": max(need, 8)}
    start, pos = {}, GUARD
    for k in sizes:
        start[k] = pos
        pos += -(-sizes[k] // GUARD) * GUARD + GUARD
    block = torch.full((pos,), SENTINEL, dtype=torch.uint8, device=DEV)
    view = {k: block[start[k]: start[k] + sizes[k]] for k in sizes}
    di = torch.tensor(image).to(DEV) if "image" in want else None
    dl = torch.tensor(labels).to(DEV) if "labels" in want else None
    check(_call(di, dl, channels, n_cls, src, dst, view["image"] if di is not None else None,
                view["labels"] if dl is not None else None, view["ws"], need), "hdf_resize_3d")
    host = block.cpu().numpy()
    assert di is None or torch.equal(di.cpu(), torch.tensor(image))
    assert dl is None or torch.equal(dl.cpu(), torch.tensor(labels))
    written = np.zeros(pos, dtype=bool)
    written[start["ws"]: start["ws"] + need] = True
    out = {}
    for k in want:
        n = sizes[k] if k == "labels" else 4 * channels * vout
        written[start[k]: start[k] + n] = True
        raw = host[start[k]: start[k] + n]
        out[k] = raw.reshape(dst) if k == "labels" else raw.view(np.float32).reshape((channels,) + tuple(dst))
    assert (host[~written] == SENTINEL).all(), "bytes outside the outputs asked for were written"
    return out


def _check_against(out, ref, image, what):
    """every output present in `out` against the restatement; prints and returns the worst image error / bound"""
    worst, share = 0.0, 0.0
    if "image" in out:
        for ch in range(image.shape[0]):
            worst = max(worst, ar.check_image(out["image"][ch], ref["image"][ch], np.abs(image[ch]).max(),
                                              "%s channel %d" % (what, ch)))
    if "labels" in out:
        share = ar.check_labels(out["labels"], ref["sums"], what)
        assert share == 0.0, share                                    # blocky labels: tests/test_resize_ref_cpu.py (b)
    print("ROUNDING resize %s image %.3f labels-excluded %.1e" % (what, worst, share), flush=True)
    return worst


# ------------------------------------------------------------------------------------------------------------- exact
def test_equal_shapes_give_a_copy():
    image, labels = _inputs(ar.SHAPE, 3, 4)
    out = _run(image, labels, 4, ar.SHAPE)
    ar.check_exact(out["image"], image, "image")
    ar.check_exact(out["labels"], np.where(labels < 4, labels, 0).astype(np.uint8), "labels")


def test_a_constant_image_stays_constant_bit_for_bit():
    src, dst = rr.SHAPES[0]
    image = np.full((2,) + src, 0.7, dtype=np.float32)
    out = _run(image, None, 2, dst, ("image",))
    ar.check_exact(out["image"], np.full((2,) + dst, 0.7, dtype=np.float32), "image")


@pytest.mark.parametrize("value", [0, 3], ids=["background", "class3"])
def test_uniform_maps_equal_the_restatement_without_exclusion(value):
    src, dst = rr.SHAPES[0]
    labels = np.full(src, value, dtype=np.uint8)
    ref = rr.resize_ref(None, labels, 4, dst)
    out = _run(None, labels, 4, dst, ("labels",))
    inner = (slice(1, -1),) * 3
    assert (ref["labels"][inner] == value).all()
    ar.check_exact(out["labels"][inner], ref["labels"][inner], "interior")
    ar.check_labels(out["labels"], ref["sums"], "whole map")
    if value == 0:
        ar.check_exact(out["labels"], np.zeros(dst, dtype=np.uint8), "background")


def test_exact_halves_are_decided_like_the_reference():
    labels = np.zeros((2, 3, 4), dtype=np.uint8)
    labels[..., :] = [1, 2, 1, 0]
    ref = rr.resize_ref(None, labels, 3, (2, 3, 6))
    assert (ref["sums"][:, ..., 1] == 0.5).all() and (ref["sums"][0, ..., 4] == 0.5).all()
    out = _run(None, labels, 3, (2, 3, 6), ("labels",))
    ar.check_exact(out["labels"], ref["labels"], "labels")          # no exclusion: >= and the last class wins
    assert (out["labels"][..., 1] == 2).all() and (out["labels"][..., 4] == 1).all()


# ---------------------------------------------------------------------------------------------------------- rounding
@pytest.mark.parametrize("channels,n_cls", [(1, 2), (1, 4), (3, 2), (3, 4)])
@pytest.mark.parametrize("src,dst", rr.SHAPES[:6], ids=IDS)
def test_resize_matches_the_restatement_to_one_rounding(src, dst, channels, n_cls):
    image, labels = _inputs(src, channels, n_cls)
    ref = _reference(src, dst, channels, n_cls)
    out = _run(image, labels, n_cls, dst)
    _check_against(out, ref, image, "%s->%s C%d n%d" % ("x".join(map(str, src)), "x".join(map(str, dst)), channels, n_cls))


@pytest.mark.parametrize("want", [("image",), ("labels",)], ids="+".join)
@pytest.mark.parametrize("src,dst", rr.SHAPES[:6], ids=IDS)
def test_image_only_and_labels_only_calls(src, dst, want):
    image, labels = _inputs(src, 3, 4)
    ref = _reference(src, dst, 3, 4)
    out = _run(image if "image" in want else None, labels if "labels" in want else None, 4, dst, want)
    assert set(out) == set(want)
    _check_against(out, ref, image, "%s->%s %s only" % ("x".join(map(str, src)), "x".join(map(str, dst)), want[0]))


def test_past_the_grid_cap():
    src, dst = rr.BIG
    assert -(-53 * 101 * 103 // 256) > 2048            # the first pass (D: 104 -> 53) writes more than 2048 blocks' worth
    image, labels = _inputs(src, 2, 3)
    ref = _reference(src, dst, 2, 3)
    out = _run(image, labels, 3, dst)
    _check_against(out, ref, image, "104x101x103->53x80x111 C2 n3")


# ------------------------------------------------------------------------------------------------------------ errors
def test_bad_arguments_are_refused_before_any_launch():
    src, dst = rr.SHAPES[0]
    image, labels = _inputs(src, 3, 4)
    vi, vo = labels.size, int(np.prod(dst))
    di, dl = torch.tensor(image).to(DEV), torch.tensor(labels).to(DEV)
    io = torch.full((3,) + dst, -3.0, device=DEV)
    lo = torch.full(dst, 77, dtype=torch.uint8, device=DEV)
    need = int(lib().hdf_resize_workspace_bytes(*src, *dst))
    ws = torch.full((need,), 77, dtype=torch.uint8, device=DEV)
    two = torch.from_numpy(np.concatenate([image.reshape(-1), image.reshape(-1)])).to(DEV)
    good = dict(image=di, labels=dl, channels=3, n_cls=4, src=src, dst=dst, io=io, lo=lo, ws=ws, ws_bytes=need)
    assert need > 0
    cases = {
        "no pair": dict(image=None, io=None, labels=None, lo=None),
        "image without image_out": dict(io=None),
        "labels_out without labels": dict(labels=None),
        "a factor above 8": dict(src=(9, 37, 43), dst=(1, 24, 48)),
        "a dimension above 1024": dict(dst=(6, 24, 1025)),
        "an empty axis": dict(dst=(6, 0, 48)),
        "one class": dict(n_cls=1),
        "nine classes": dict(n_cls=9),
        "65 channels": dict(channels=65),
        "a workspace one byte short": dict(ws_bytes=need - 1),
        "a null workspace": dict(ws=None),
        "image_out is the image": dict(io=di),
        "labels_out is the labels": dict(lo=dl),
        "image_out overlaps the image's tail": dict(image=two[:3 * vi], io=two[3 * vi - 1: 3 * vi - 1 + 3 * vo]),
        "labels_out inside the workspace": dict(lo=ws[8:]),
        "the workspace is the image": dict(ws=di),
    }
    for what, kw in cases.items():
        k = {**good, **kw}
        rc = _call(k["image"], k["labels"], k["channels"], k["n_cls"], k["src"], k["dst"], k["io"], k["lo"], k["ws"],
                   k["ws_bytes"])
        assert rc != 0 and lib().hdf_last_error().startswith(b"resize_3d:"), (what, rc, lib().hdf_last_error())
    vol = torch.full((64,), 5.0, device=DEV)
    for what, (t, n, a, b) in {"hi == lo": (vol, 64, 1.0, 1.0), "hi < lo": (vol, 64, 2.0, 1.0),
                               "nan": (vol, 64, float("nan"), 1.0), "inf": (vol, 64, 0.0, float("inf")),
                               "nothing": (vol, 0, 0.0, 1.0), "null": (None, 64, 0.0, 1.0)}.items():
        rc = lib().hdf_trunc_normalize(ptr(t), n, a, b, st())
        assert rc != 0 and lib().hdf_last_error().startswith(b"trunc_normalize:"), (what, rc, lib().hdf_last_error())
    torch.cuda.synchronize()
    assert torch.equal(di.cpu(), torch.tensor(image)) and torch.equal(dl.cpu(), torch.tensor(labels))
    assert bool((io == -3.0).all()) and bool((lo == 77).all()) and bool((ws == 77).all()) and bool((vol == 5.0).all())
    assert torch.equal(two[:3 * vi].cpu().reshape(image.shape), torch.tensor(image))
    assert _call(di, dl, 3, 4, src, dst, io, lo, ws, need) == 0                  # and the good set is accepted


def test_resize_3d_refuses_a_wrong_tensor_before_the_call():
    """every tensor the kernel writes through is checked for device, dtype, shape and contiguity in Python: the C entry
    sees only addresses"""
    from hdf_rt import crop_resize, resize_3d, trunc_normalize_
    src, dst = rr.SHAPES[0]
    image, labels = _inputs(src, 3, 4)
    di, dl = torch.tensor(image).to(DEV), torch.tensor(labels).to(DEV)
    good = {"out_image": torch.full((3,) + dst, -3.0, device=DEV),
            "out_labels": torch.full(dst, 77, dtype=torch.uint8, device=DEV)}
    wide = torch.full(dst[:2] + (2 * dst[2],), 77, dtype=torch.uint8, device=DEV)
    bad = {
        "out_labels": {"int64": torch.full(dst, 77, dtype=torch.int64, device=DEV),
                       "too small": torch.full(dst[:2] + (dst[2] - 1,), 77, dtype=torch.uint8, device=DEV),
                       "flat": torch.full((int(np.prod(dst)),), 77, dtype=torch.uint8, device=DEV),
                       "strided": wide[:, :, ::2],
                       "host": torch.full(dst, 77, dtype=torch.uint8),
                       "not a tensor": np.zeros(dst, dtype=np.uint8)},
        "out_image": {"half": torch.full((3,) + dst, -3.0, dtype=torch.float16, device=DEV),
                      "one channel short": torch.full((2,) + dst, -3.0, device=DEV),
                      "strided": torch.full((3,) + dst[:2] + (2 * dst[2],), -3.0, device=DEV)[..., ::2],
                      "host": torch.full((3,) + dst, -3.0)},
    }
    for arg, cases in bad.items():
        for what, t in cases.items():
            with pytest.raises(ValueError, match=arg):
                resize_3d(di, dl, 4, dst, **{**good, arg: t})
            if torch.is_tensor(t):
                assert bool((t == (77 if t.dtype in (torch.uint8, torch.int64) else -3.0)).all()), (arg, what)
    with pytest.raises(ValueError, match="labels must be"):
        resize_3d(di, dl.long(), 4, dst)
    with pytest.raises(ValueError, match="labels must be"):
        resize_3d(di, dl[:, :, 1:], 4, dst)
    with pytest.raises(ValueError, match="image must be"):
        resize_3d(di.double(), dl, 4, dst)
    with pytest.raises(ValueError, match="out_shape must be"):
        resize_3d(di, dl, 4, dst[:2])
    with pytest.raises(ValueError, match="out_image needs an image"):
        resize_3d(None, dl, 4, dst, out_image=good["out_image"])
    with pytest.raises(ValueError, match="outside the kernel's limits"):
        resize_3d(di, dl, 4, (1, 24, 48))
    with pytest.raises(ValueError, match="image must be a contiguous float32"):
        trunc_normalize_(di[..., ::2], (0, 1))
    with pytest.raises(ValueError, match="scale must be"):
        trunc_normalize_(di, (0, 1, 2))
    torch.cuda.synchronize()
    assert bool((wide == 77).all()) and torch.equal(di.cpu(), torch.tensor(image))
    assert bool((good["out_image"] == -3.0).all()) and bool((good["out_labels"] == 77).all())
    r_i, r_l = resize_3d(di, dl, 4, dst, **good)                                 # and the good set is accepted
    assert r_i.data_ptr() == good["out_image"].data_ptr() and r_l.data_ptr() == good["out_labels"].data_ptr()
    ref = _reference(src, dst, 3, 4)
    _check_against({"image": r_i.cpu().numpy(), "labels": r_l.cpu().numpy()}, ref, image, "resize_3d into given tensors")
    # crop_resize: the H/W crop is a slice, a sample already at `dim` comes back as it is, a 2-D sample goes through
    c_i, c_l = crop_resize(di, dl, 4, (9, 33, 39), crop=2)
    assert c_i.data_ptr() == di[..., 2:-2, 2:-2].data_ptr() and c_l.shape == (9, 33, 39)
    p_i, p_l = crop_resize(di[:, 0], dl[0], 4, (24, 48))
    q_i, q_l = resize_3d(di[:, :1], dl[:1], 4, (1, 24, 48))
    assert p_i.shape == (3, 24, 48) and torch.equal(p_i, q_i[:, 0]) and torch.equal(p_l, q_l[0])


# -------------------------------------------------------------------------------------------------- trunc_normalize_
def test_trunc_normalize_is_numpys_fp32_sequence():
    from hdf_rt import trunc_normalize_
    rng = np.random.RandomState(5)
    vol = (rng.standard_normal((1, 7, 33, 41)) * 400.0 - 50.0).astype(np.float32)          # CT-like: both sides of the window
    lo, hi = -100, 200
    vol.reshape(-1)[:4] = [lo, hi, np.nextafter(np.float32(lo), np.float32(0)), np.nextafter(np.float32(hi), np.float32(0))]
    assert (vol < lo).mean() > 0.2 and (vol > hi).mean() > 0.2
    want = vol - lo                                                                        # data_loader.py:28-33
    gray_range = hi - lo
    want[want < 0] = 0
    want[want > gray_range] = gray_range
    want = want / gray_range
    assert want.dtype == np.float32 and want.reshape(-1)[0] == 0.0 and want.reshape(-1)[1] == 1.0
    t = torch.tensor(vol).to(DEV)
    assert trunc_normalize_(t, (lo, hi)) is t
    ar.check_exact(t.cpu().numpy(), want, "trunc_normalize_")
    odd = torch.tensor(vol.reshape(-1)[:1001] * 1.5).to(DEV)                                # a non-integer window
    w2 = odd.cpu().numpy() - np.float32(-12.5)
    w2[w2 < 0] = 0
    w2[w2 > np.float32(83.25)] = np.float32(83.25)
    ar.check_exact(trunc_normalize_(odd, (-12.5, 70.75)).cpu().numpy(), w2 / np.float32(83.25), "odd window")


# ------------------------------------------------------------------------------------------------ the Python chain
def _raw_sample():
    rng = np.random.RandomState(21)
    image = rng.standard_normal((2, 20, 45, 50)).astype(np.float32)
    image[0] *= 700.0                                                # CT-like range: the clip of PETandCTNormalize bites
    labels = ar.labels_of((20, 45, 50), 3, 21, blocky=True)
    return torch.tensor(image).to(DEV), torch.tensor(labels).to(DEV)


def test_from_ids_is_the_chain_of_its_parts_under_the_same_draws():
    from hdf_rt import TrainTransform3D, augment_3d, crop_resize, flip_flags, trz_matrix
    from hdf_rt.inference import pet_ct_normalize_
    image, labels = _raw_sample()
    keep_i, keep_l = image.clone(), labels.clone()
    dim = (16, 32, 48)
    tf = TrainTransform3D.from_ids(3, [2, 3, 4, 5, 6], input_shape=dim)
    for seed in (0, 1):
        random.seed(seed), np.random.seed(seed)
        got_i, got_oh = tf(image, labels)
        assert torch.equal(image, keep_i) and torch.equal(labels, keep_l)        # the arguments are left alone
        random.seed(seed), np.random.seed(seed)
        ni = pet_ct_normalize_(image.clone())
        ri, rl = crop_resize(ni, labels, 3, dim)
        aff, (fh, fw) = trz_matrix("tr"), flip_flags("hv")
        want_i, want_oh = augment_3d(ri, rl, 3, aff, fh, fw)
        assert got_i.shape == (2,) + dim and got_oh.shape == (3,) + dim
        assert torch.equal(got_i, want_i) and torch.equal(got_oh, want_oh)
        # and the parts are the restatements': the resize of the normalised volume, then its warp
        ref = rr.resize_ref(ni.cpu().numpy(), labels.cpu().numpy(), 3, dim)
        _check_against({"image": ri.cpu().numpy(), "labels": rl.cpu().numpy()}, ref, ni.cpu().numpy(),
                       "from_ids resize seed %d" % seed)
    # the margin of CropResize and a trailing Trunc_and_Normalize
    random.seed(2), np.random.seed(2)
    got_i, got_oh = TrainTransform3D.from_ids(3, [2, 3, 4, 5, 6, 7], input_shape=dim, crop=3, scale=(-1, 2))(image, labels)
    random.seed(2), np.random.seed(2)
    from hdf_rt import trunc_normalize_
    ri, rl = crop_resize(pet_ct_normalize_(image.clone()), labels, 3, dim, crop=3)
    want_i, want_oh = augment_3d(ri.contiguous(), rl.contiguous(), 3, trz_matrix("tr"), *flip_flags("hv"))
    assert torch.equal(got_i, trunc_normalize_(want_i, (-1, 2))) and torch.equal(got_oh, want_oh)
    assert float(got_i.min()) >= 0.0 and float(got_i.max()) <= 1.0


def test_validation_form_is_normalise_resize_onehot():
    from hdf_rt import TrainTransform3D, crop_resize
    from hdf_rt.inference import onehot_from_labels, pet_ct_normalize_
    image, labels = _raw_sample()
    dim = (16, 32, 48)
    random.seed(4)
    state = (random.getstate(), np.random.get_state()[1].copy())
    got_i, got_oh = TrainTransform3D.from_ids(3, [2, 3, 4, 5, 6], input_shape=dim, train=False)(image, labels)
    assert random.getstate() == state[0] and np.array_equal(np.random.get_state()[1], state[1])      # no draw at all
    ri, rl = crop_resize(pet_ct_normalize_(image.clone()), labels, 3, dim)
    assert torch.equal(got_i, ri) and torch.equal(got_oh, onehot_from_labels(rl[None], 3)[0])


def test_the_chain_goes_straight_into_the_model_and_the_loss():
    from hdf_rt import TrainTransform3D
    from loss.combine_loss import CEPlusDice, DeepSuperloss
    from models.HDenseFormer import HDenseFormer
    image, labels = _raw_sample()
    dim = (32, 32, 48)                                  # the smallest depth the model takes
    random.seed(0), np.random.seed(0)
    x, onehot = TrainTransform3D.from_ids(3, [2, 3, 4, 5, 6], input_shape=dim)(image, labels)
    for t, c in ((x, 2), (onehot, 3)):                  # what the model and the loss take as they are
        assert t.dtype == torch.float32 and t.is_contiguous() and t.device.type == "cuda" and tuple(t.shape) == (c,) + dim
    assert bool((onehot.sum(0) == 1).all())
    torch.manual_seed(0)
    net = HDenseFormer(2, 3, 16, image_size=dim, transformer_depth=8).to(DEV).train()
    outs = net(x[None])
    loss = DeepSuperloss(criterion=CEPlusDice(weight=None, ignore_index=0))(outs, onehot[None])
    loss.backward()
    torch.cuda.synchronize()
    assert tuple(outs[0].shape) == (1, 3) + dim and bool(torch.isfinite(loss))
    grads = [p.grad for p in net.parameters() if p.grad is not None]
    assert grads and all(bool(torch.isfinite(g).all()) for g in grads)
