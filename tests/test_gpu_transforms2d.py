"""hdf_label_bbox_2d, hdf_zoom_2d and hdf_intensity_2d (include/hdf.h, csrc/augment.hip) called directly through ctypes.
  bbox: exact against numpy (batch 5 of 37x43 with an empty, a single-pixel and a full sample; one 600x600 plane, past
      one workgroup's share)
  zoom: BIT FOR BIT tests/zoom2d_ref.py, the numpy restatement of PIL's crop / expand + resize (itself held to PIL by
      tests/test_zoom2d_ref_cpu.py): image elements compared as uint32, labels as bytes, no tolerance.  Every call writes
      into one sentinel-filled block with guard bands around the two outputs: an output not asked for, and every guard,
      must come back untouched, and the sources unchanged.  Batch 5 at 37x43 and 43x37 with a canvas and a keep-rectangle
      per sample (factors 0.8, 1.0, 1.2, an off-plane crop, erase-all, erase without zoom); 33 samples at 24x24 (two
      parameter chunks); 1x1, 1x9, 9x1; the canvas limits W/4 and 4W; image-only and label-only calls; every refusal
      before any launch
  intensity: gamma within ONE fp32 ulp of float32(np.power(float64(x), float64(float32(gamma)))) -- the device's and
      numpy's fp64 pow may differ in the last fp64 bit, which moves the fp32 rounding only at a tie -- with 0 and 1 exact
      and gamma 1 leaving the bits; noise deterministic in (seed, sample, element), held to the normal CDF by the DKW bound
      at alpha = 1e-9, uncorrelated between samples, clipped to [0, 1], and within one fp32 ulp of the restatement's
      Philox + Box-Muller field
  the chain: TrainTransform2D.from_ids(2, [1,3,4,6,7,8,9,10]) equals its parts called by hand under the same draws, goes
      straight into models.HDenseFormer_2D and the loss, and from_ids(train=False) is the validation form."""
import ctypes as C
import functools
import math
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import zoom2d_ref as zr  # noqa: E402
from hdf_rt._lib import check, lib, ptr  # noqa: E402
from hip_util import DEV, st  # noqa: E402

SENTINEL = 0xA5
GUARD = 1024
CHUNK = 32            # samples per launch (csrc/augment.h AUG2D_CHUNK)


# -------------------------------------------------------------------------------------------------------------- bbox
def _bbox(labels):
    d = torch.tensor(labels).to(DEV)
    b, h, w = labels.shape
    nbytes = lib().hdf_label_bbox_workspace_bytes(b)
    ws = torch.full((nbytes + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device=DEV)
    out = torch.full((b * 5 + 2 * GUARD // 4,), -7, dtype=torch.int32, device=DEV)
    check(lib().hdf_label_bbox_2d(ptr(d), b, h, w, out.data_ptr() + GUARD, ws.data_ptr() + GUARD, nbytes, st()),
          "hdf_label_bbox_2d")
    assert torch.equal(d.cpu(), torch.tensor(labels))
    host, wsh = out.cpu().numpy(), ws.cpu().numpy()
    assert (host[:GUARD // 4] == -7).all() and (host[GUARD // 4 + b * 5:] == -7).all()
    assert (wsh[:GUARD] == SENTINEL).all() and (wsh[GUARD + nbytes:] == SENTINEL).all()
    return host[GUARD // 4: GUARD // 4 + b * 5].reshape(b, 5)


def test_bbox_of_a_batch_is_exact():
    shape = (37, 43)
    labels = np.stack([zr.labels_of(shape, 3), np.zeros(shape, np.uint8), np.zeros(shape, np.uint8),
                       np.full(shape, 2, np.uint8), np.zeros(shape, np.uint8)])
    labels[2, 36, 42] = 255                                           # a single pixel, the last of its plane
    labels[4, 5:9, 11:30] = 1
    want = zr.bbox_ref(labels)
    assert want[1].tolist() == [0, 37, -1, 43, -1] and want[2].tolist() == [1, 36, 36, 42, 42]
    assert want[3].tolist() == [37 * 43, 0, 36, 0, 42] and want[4].tolist() == [76, 5, 8, 11, 29]
    got = _bbox(labels)
    assert got.dtype == np.int32 and np.array_equal(got, want), (got, want)


def test_bbox_of_a_plane_past_one_workgroups_share():
    labels = np.zeros((1, 600, 600), np.uint8)
    rng = np.random.RandomState(2)
    rows, cols = rng.randint(17, 590, 300), rng.randint(23, 577, 300)
    labels[0, rows, cols] = rng.randint(1, 256, 300)
    labels[0, 599, 3] = 1                                             # the extremes lie in different blocks' shares
    want = zr.bbox_ref(labels)
    assert want[0, 2] == 599 and want[0, 3] == 3
    assert np.array_equal(_bbox(labels), want)


def test_bbox_refusals():
    d = torch.zeros((2, 5, 7), dtype=torch.uint8, device=DEV)
    out = torch.full((10,), -7, dtype=torch.int32, device=DEV)
    nbytes = lib().hdf_label_bbox_workspace_bytes(2)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    for what, args in {"null labels": (None, 2, 5, 7, ptr(out), ptr(ws), nbytes),
                       "null bbox": (ptr(d), 2, 5, 7, None, ptr(ws), nbytes),
                       "null workspace": (ptr(d), 2, 5, 7, ptr(out), None, nbytes),
                       "short workspace": (ptr(d), 2, 5, 7, ptr(out), ptr(ws), nbytes - 1),
                       "no sample": (ptr(d), 0, 5, 7, ptr(out), ptr(ws), nbytes),
                       "zero height": (ptr(d), 2, 0, 7, ptr(out), ptr(ws), nbytes),
                       "too wide": (ptr(d), 2, 5, 16385, ptr(out), ptr(ws), 1 << 30)}.items():
        rc = lib().hdf_label_bbox_2d(*args, st())
        assert rc != 0 and lib().hdf_last_error().startswith(b"label_bbox_2d:"), (what, rc, lib().hdf_last_error())
    torch.cuda.synchronize()
    assert bool((out == -7).all())


# -------------------------------------------------------------------------------------------------------------- zoom
@functools.lru_cache(maxsize=None)
def _inputs(batch, channels, shape, seed=1):
    image = np.stack([zr.image_of(shape, channels, seed + 10 * b) for b in range(batch)])
    image[:, -1] *= 1000.0
    labels = np.stack([zr.labels_of(shape, seed + 10 * b, blocky=False) for b in range(batch)])
    image.setflags(write=False), labels.setflags(write=False)
    return image, labels


@functools.lru_cache(maxsize=None)
def _reference(batch, channels, shape, keeps, canvases, seed=1):
    image, labels = _inputs(batch, channels, shape, seed)
    ref = zr.zoom2d_batch_ref(image, labels, keeps, canvases)
    for v in ref.values():
        v.setflags(write=False)
    return ref


def _rows(rows):
    return None if rows is None else np.ascontiguousarray(rows, dtype=np.int32).reshape(-1, 4)


def _call(image, labels, batch, channels, shape, keeps, canvases, io, lo):
    k, c = _rows(keeps), _rows(canvases)
    return lib().hdf_zoom_2d(ptr(image), ptr(labels), batch, channels, shape[0], shape[1],
                             None if k is None else k.ctypes.data, None if c is None else c.ctypes.data, ptr(io), ptr(lo),
                             st())


def _run(image, labels, keeps, canvases, want=("image", "labels")):
    """one call on host arrays [B, C, H, W] / [B, H, W]; returns {name: numpy array} of the outputs asked for, after
    checking that everything else in the output block still holds the sentinel and that the sources are unchanged"""
    batch, channels, shape = image.shape[0], image.shape[1], tuple(image.shape[2:])
    pix = batch * shape[0] * shape[1]
    sizes = {"image": 4 * channels * pix, "labels": pix}
    start, pos = {}, GUARD
    for k in sizes:
        start[k] = pos
        pos += -(-sizes[k] // GUARD) * GUARD + GUARD
    block = torch.full((pos,), SENTINEL, dtype=torch.uint8, device=DEV)
    view = {k: block[start[k]: start[k] + sizes[k]] for k in sizes}
    di, dl = torch.tensor(image).to(DEV), torch.tensor(labels).to(DEV)
    check(_call(di, dl, batch, channels, shape, keeps, canvases, *[view[k] if k in want else None for k in sizes]),
          "hdf_zoom_2d")
    host = block.cpu().numpy()
    zr.check_exact(di.cpu().numpy(), np.asarray(image), "the source image")      # as bits: a NaN equals itself
    assert torch.equal(dl.cpu(), torch.tensor(labels))
    written = np.zeros(pos, dtype=bool)
    out = {}
    for k in want:
        written[start[k]: start[k] + sizes[k]] = True
        raw = host[start[k]: start[k] + sizes[k]]
        out[k] = (raw.reshape((batch,) + shape) if k == "labels"
                  else raw.view(np.float32).reshape((batch, channels) + shape))
    assert (host[~written] == SENTINEL).all(), "bytes outside the outputs asked for were written"
    return out


def _check_against(out, ref, what):
    for k in out:
        zr.check_exact(out[k], ref[k], "%s %s" % (what, k))


def _batch_params(shape):
    """five samples: a crop at 0.8 inside the plane with an erased top; factor 1.0 with an erased right (erase without
    zoom); a pad at 1.2 with a shifted paste; a crop at 0.8 that leaves the plane on two sides; erase-all under a pad"""
    h, w = shape
    tw8, th8, tw12, th12 = int(w * 0.8), int(h * 0.8), int(w * 1.2), int(h * 1.2)
    canvases = (zr.crop_canvas(3, 2, tw8, th8), (w, h, 0, 0), zr.expand_canvas(4, 3, tw12, th12),
                zr.crop_canvas(w - tw8 + 4, -2, tw8, th8), zr.expand_canvas(0, 1, tw12, th12))
    keeps = ((6, h, 0, w), (0, h, 0, w - 9), zr.full_keep(h, w), (0, h - 5, 4, w), (0, 0, 0, w))
    return keeps, canvases


@pytest.mark.parametrize("shape", [(37, 43), (43, 37)], ids=["37x43", "43x37"])
def test_batch_with_a_canvas_and_a_keep_rectangle_per_sample_is_exact(shape):
    keeps, canvases = _batch_params(shape)
    image, labels = _inputs(5, 2, shape)
    assert {0, 1, 2, 3, 200, 255} <= set(np.unique(labels).tolist()) and (image < 0).any()
    ref = _reference(5, 2, shape, keeps, canvases)
    assert not ref["image"][4].any() and ref["labels"][4].any()      # erase-all: the image only
    assert np.array_equal(ref["labels"][1], labels[1])               # factor 1.0: the labels pass through
    assert (ref["labels"][3] == 0).mean() > 0.05                     # the off-plane crop brought zeros in
    out = _run(image, labels, keeps, canvases)
    _check_against(out, ref, "batch %dx%d" % shape)
    # erase without zoom is the erase itself, -0.0 and all: no arithmetic touches a skipped pass
    zr.check_exact(out["image"][1], zr.erase(image[1], keeps[1]), "erase alone")


def test_skipped_passes_move_the_bits_unchanged():
    shape = (37, 43)
    image, labels = _inputs(2, 2, shape)
    image = image.copy()
    image[0, 0, 3, 4], image[0, 0, 5, 6], image[1, 1, 0, 0] = -0.0, np.inf, np.nan
    keeps, canvases = (zr.full_keep(*shape),) * 2, ((43, 37, 0, 0),) * 2
    out = _run(image, labels, keeps, canvases)
    zr.check_exact(out["image"], image, "identity image")
    zr.check_exact(out["labels"], labels, "identity labels")
    # one pass each: the width alone, then the height alone
    keeps, canvases = (zr.full_keep(*shape),) * 2, ((51, 37, 2, 0), (43, 30, 0, -3))
    image, labels = _inputs(2, 2, shape)
    _check_against(_run(image, labels, keeps, canvases), _reference(2, 2, shape, keeps, canvases), "one pass")


def test_more_samples_than_one_parameter_chunk():
    shape, batch = (24, 24), CHUNK + 1
    canvases = tuple(zr.crop_canvas(b % 5, b % 3, 19 + b % 4, 19 + b % 5) if b % 2 else
                     zr.expand_canvas(b % 4, b % 3, 25 + b % 4, 26 + b % 3) for b in range(batch))
    keeps = tuple((b % 7, 24 - b % 3, b % 5, 24 - b % 2) for b in range(batch))
    image, labels = _inputs(batch, 2, shape)
    ref = _reference(batch, 2, shape, keeps, canvases)
    out = _run(image, labels, keeps, canvases)
    _check_against(out, ref, "%d samples" % batch)
    assert canvases[CHUNK] != canvases[CHUNK - 1] and keeps[CHUNK] != keeps[CHUNK - 1]
    assert not np.array_equal(ref["image"][CHUNK], ref["image"][CHUNK - 1])


@pytest.mark.parametrize("shape", [(1, 1), (1, 9), (9, 1)], ids=lambda s: "%dx%d" % s)
def test_degenerate_shapes(shape):
    h, w = shape
    canvases = ((w, h, 0, 0), (2 * w, h + 1, 1, 0), (max(w - 2, 1), max(h - 2, 1), -1, -1), (4 * w, 4 * h, w, h),
                (-(-w // 4), -(-h // 4), 0, 0))
    keeps = (zr.full_keep(h, w), zr.full_keep(h, w), zr.full_keep(h, w), (0, h, 0, w), (0, h, 0, max(w - 1, 0)))
    image, labels = _inputs(5, 2, shape)
    ref = _reference(5, 2, shape, keeps, canvases)
    _check_against(_run(image, labels, keeps, canvases), ref, "%dx%d" % shape)


def test_the_canvas_limits_are_exact():
    """W/4 and 4W: one tap against nine, the widest support the entry lets through (factors 0.5 and 2.0 on the way)"""
    shape = (24, 28)
    canvases = ((7, 6, -3, -2), (112, 96, 40, 30), (14, 12, 0, 0), (56, 48, 0, 0), (7, 96, 0, 30))
    keeps = (zr.full_keep(*shape),) * 4 + ((2, 20, 3, 25),)
    image, labels = _inputs(5, 2, shape)
    ref = _reference(5, 2, shape, keeps, canvases)
    _check_against(_run(image, labels, keeps, canvases), ref, "canvas limits")


def test_image_only_and_label_only_calls():
    shape = (37, 43)
    keeps, canvases = _batch_params(shape)
    image, labels = _inputs(5, 2, shape)
    ref = _reference(5, 2, shape, keeps, canvases)
    for want in (("image",), ("labels",)):                           # the other output stays untouched
        out = _run(image, labels, keeps, canvases, want)
        assert set(out) == set(want)
        _check_against(out, ref, "+".join(want))
    di, dl = torch.tensor(image).to(DEV), torch.tensor(labels).to(DEV)
    io = torch.empty_like(di)
    check(_call(di, None, 5, 2, shape, keeps, canvases, io, None), "hdf_zoom_2d")          # null labels
    zr.check_exact(io.cpu().numpy(), ref["image"], "image")
    lo = torch.empty_like(dl)
    check(_call(None, dl, 5, 0, shape, keeps, canvases, None, lo), "hdf_zoom_2d")          # null image, no channel
    zr.check_exact(lo.cpu().numpy(), ref["labels"], "labels")


def test_bad_arguments_are_refused_before_any_launch():
    shape = (37, 43)
    h, w = shape
    keeps, canvases = (np.array(v, dtype=np.int32) for v in _batch_params(shape))
    image, labels = _inputs(5, 2, shape)
    pix = labels.size
    di, dl = torch.tensor(image).to(DEV), torch.tensor(labels).to(DEV)
    io = torch.full((5, 2) + shape, -3.0, device=DEV)
    lo = torch.full((5,) + shape, 77, dtype=torch.uint8, device=DEV)
    two = torch.from_numpy(np.concatenate([image.reshape(-1), image.reshape(-1)])).to(DEV)
    both = torch.full((9 * pix,), 77, dtype=torch.uint8, device=DEV)

    def canvas_with(b, k, v):
        c = canvases.copy()
        c[b, k] = v
        return c

    def keep_with(b, row):
        k = keeps.copy()
        k[b] = row
        return k

    cases = {
        "image_out is the image": dict(io=di),
        "labels_out is the labels": dict(lo=dl),
        "image_out overlaps the image's tail": dict(image=two[:2 * pix], io=two[2 * pix - 1: 4 * pix - 1]),
        "labels_out overlaps the image": dict(lo=di.view(torch.uint8).reshape(-1)[8:8 + pix]),
        "the outputs overlap": dict(io=both[:8 * pix].view(torch.float32), lo=both[8 * pix - 4: 9 * pix - 4]),
        "no output": dict(io=None, lo=None),
        "an image output without an image": dict(image=None),
        "a label output without labels": dict(labels=None),
        "null keep": dict(keeps=None),
        "null canvas": dict(canvases=None),
        "canvas too narrow": dict(canvases=canvas_with(1, 0, -(-w // 4) - 1)),
        "canvas too wide": dict(canvases=canvas_with(2, 0, 4 * w + 1)),
        "canvas too low": dict(canvases=canvas_with(3, 1, -(-h // 4) - 1)),
        "canvas too high": dict(canvases=canvas_with(4, 1, 4 * h + 1)),
        "canvas of no width": dict(canvases=canvas_with(0, 0, 0)),
        "canvas far away": dict(canvases=canvas_with(0, 2, 1 << 20)),
        "keep past the bottom": dict(keeps=keep_with(1, (0, h + 1, 0, w))),
        "keep past the right": dict(keeps=keep_with(2, (0, h, 0, w + 1))),
        "keep with a negative row": dict(keeps=keep_with(3, (-1, h, 0, w))),
        "keep reversed": dict(keeps=keep_with(4, (9, 8, 0, w))),
        "no sample": dict(batch=0),
        "zero height": dict(shape=(0, 43)),
        "negative width": dict(shape=(37, -1)),
        "too wide": dict(shape=(1, 16385)),
        "65 channels": dict(channels=65),
        "no channel": dict(channels=0),
    }
    for what, over in cases.items():
        a = dict(image=di, labels=dl, batch=5, channels=2, shape=shape, keeps=keeps, canvases=canvases, io=io, lo=lo)
        a.update(over)
        rc = _call(a["image"], a["labels"], a["batch"], a["channels"], a["shape"], a["keeps"], a["canvases"], a["io"],
                   a["lo"])
        assert rc != 0 and lib().hdf_last_error().startswith(b"zoom_2d:"), (what, rc, lib().hdf_last_error())
        if what == "canvas too wide":
            assert lib().hdf_last_error().startswith(b"zoom_2d: canvas[2] is 173 wide")
        if what == "keep reversed":
            assert lib().hdf_last_error().startswith(b"zoom_2d: keep[4]")
    torch.cuda.synchronize()
    assert torch.equal(di.cpu(), torch.tensor(image)) and torch.equal(dl.cpu(), torch.tensor(labels))
    assert bool((io == -3.0).all()) and bool((lo == 77).all()) and bool((both == 77).all())
    assert torch.equal(two[:2 * pix].cpu().reshape(image.shape), torch.tensor(image))


def test_zoom_2d_wrapper_checks_its_tensors_and_returns_both_outputs():
    from hdf_rt import zoom_2d
    shape = (37, 43)
    keeps, canvases = _batch_params(shape)
    image, labels = _inputs(5, 2, shape)
    ref = _reference(5, 2, shape, keeps, canvases)
    di, dl = torch.tensor(image).to(DEV), torch.tensor(labels).to(DEV)
    got_i, got_l = zoom_2d(di, dl, keeps, canvases)
    _check_against({"image": got_i.cpu().numpy(), "labels": got_l.cpu().numpy()}, ref, "zoom_2d")
    only_i, none = zoom_2d(di, None, keeps, canvases)
    assert none is None and torch.equal(only_i, got_i)
    with pytest.raises(ValueError, match="keeps must be"):
        zoom_2d(di, dl, keeps[:4], canvases)
    with pytest.raises(ValueError, match="canvases must be"):
        zoom_2d(di, dl, keeps, [(43.5, 37, 0, 0)] * 5)
    with pytest.raises(ValueError, match="out_labels"):
        zoom_2d(di, dl, keeps, canvases, out_labels=torch.empty((5, 37, 42), dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match="out_image"):
        zoom_2d(di, dl, keeps, canvases, out_image=torch.empty((5, 2, 37, 43), dtype=torch.float16, device=DEV))
    with pytest.raises(ValueError, match="labels must be"):
        zoom_2d(di, dl[:4], keeps, canvases)


# --------------------------------------------------------------------------------------------------------- intensity
def _intensity(x, gammas, noise, seed=0, low_clip=0.0):
    """one call in place on a host array [B, C, H, W] between guard bands; returns the result"""
    b, c, h, w = x.shape
    block = torch.full((x.size + 2 * GUARD // 4,), -3.0, dtype=torch.float32, device=DEV)
    body = block[GUARD // 4: GUARD // 4 + x.size]
    body.copy_(torch.tensor(x).reshape(-1))
    g = np.ascontiguousarray(gammas, dtype=np.float64)
    f = np.ascontiguousarray(noise, dtype=np.uint8)
    check(lib().hdf_intensity_2d(ptr(body), b, c, h, w, g.ctypes.data_as(C.POINTER(C.c_double)), f.ctypes.data, seed,
                                 low_clip, st()), "hdf_intensity_2d")
    host = block.cpu().numpy()
    assert (host[:GUARD // 4] == -3.0).all() and (host[GUARD // 4 + x.size:] == -3.0).all()
    return host[GUARD // 4: GUARD // 4 + x.size].reshape(x.shape)


def _ulps(got, want):
    """distance in fp32 steps between two arrays of non-negative floats"""
    return np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))


def test_gamma_is_pow_in_fp64_rounded_once():
    rng = np.random.RandomState(5)
    x = rng.uniform(0, 1, (CHUNK + 2, 2, 17, 29)).astype(np.float32)          # two parameter chunks
    x[:, 0, 0, :4] = (0.0, 1.0, np.float32(1e-30), np.nextafter(np.float32(1), np.float32(0)))
    gammas = [0.8 + 0.4 * k / (CHUNK + 1) for k in range(CHUNK + 2)]
    gammas[3], gammas[CHUNK] = 1.0, 1.0
    x[3, 1, 2, 2] = -0.25                                                     # gamma 1 leaves even a negative alone
    got = _intensity(x, gammas, [0] * len(gammas))
    worst = 0
    for b, g in enumerate(gammas):
        want = zr.gamma_ref(x[b], g)
        if g == 1.0:
            zr.check_exact(got[b], x[b], "gamma 1, sample %d" % b)
            continue
        d = _ulps(got[b], want)
        worst = max(worst, int(d.max()))
        assert d.max() <= 1, (b, g, int(d.max()))
        assert got[b, 0, 0, 0] == 0.0 and got[b, 0, 0, 1] == 1.0             # 0 and 1 are exact
    print("gamma: worst distance %d ulp over %d elements" % (worst, x.size))
    neg = np.array([[[[-0.5, 0.0, 0.25, -0.0]]]], dtype=np.float32)
    assert _intensity(neg, [0.5], [0]).reshape(-1).tolist() == [0.0, 0.0, 0.5, 0.0]


NOISE_SHAPE = (4, 2, 64, 64)


@functools.lru_cache(maxsize=None)
def _noise_field(seed, low_clip=-1.0, base=0.0, flags=(1, 1, 1, 1)):
    out = _intensity(np.full(NOISE_SHAPE, base, dtype=np.float32), [1.0] * 4, flags, seed, low_clip)
    out.setflags(write=False)
    return out


def test_noise_is_a_function_of_seed_sample_and_element():
    a = _noise_field(1234567890123)
    zr.check_exact(_intensity(np.zeros(NOISE_SHAPE, np.float32), [1.0] * 4, [1] * 4, 1234567890123, -1.0), a, "same seed")
    assert not np.array_equal(a, _noise_field(1234567890124))                 # another seed
    assert not np.array_equal(a, _noise_field(1234567890123 + (1 << 32)))     # its high word counts too
    for b in range(1, 4):
        assert not np.array_equal(a[0], a[b])                                 # another sample
    assert not np.array_equal(a[0, 0], a[0, 1])                               # another channel
    # a sample's field depends neither on the batch around it nor on the launch geometry (the same elements as one row)
    part = _noise_field(1234567890123, flags=(0, 1, 0, 1))
    assert not part[0].any() and not part[2].any()                            # noise[b] = 0 leaves sample b untouched
    zr.check_exact(part[1], a[1], "sample 1")
    zr.check_exact(part[3], a[3], "sample 3")
    flat = _intensity(np.zeros((2, 1, 1, 2 * 64 * 64), np.float32), [1.0] * 2, [1] * 2, 1234567890123, -1.0)
    zr.check_exact(flat.reshape(2, -1), a[:2].reshape(2, -1), "another geometry")


def test_noise_is_standard_normal_times_a_tenth():
    out = _noise_field(99)
    n = out.size
    assert n == 4 * 2 * 64 * 64
    z = np.sort(out.reshape(-1).astype(np.float64) / 0.1)
    cdf = torch.special.ndtr(torch.tensor(z)).numpy()
    d = max(np.abs(cdf - np.arange(1, n + 1) / n).max(), np.abs(cdf - np.arange(n) / n).max())
    bound = math.sqrt(math.log(2 / 1e-9) / (2 * n))                           # DKW at alpha = 1e-9
    print("noise: sup |F_n - Phi| = %.5f (bound %.5f), mean %.5f, std %.5f" % (d, bound, z.mean(), z.std()))
    assert d < bound
    s0, s1 = out[0].reshape(-1).astype(np.float64), out[1].reshape(-1).astype(np.float64)
    corr = float(np.corrcoef(s0, s1)[0, 1])
    print("noise: correlation of samples 0 and 1 = %.5f (bound %.5f)" % (corr, 6 / math.sqrt(n / 4)))
    assert abs(corr) < 6 / math.sqrt(n / 4)


def test_noise_is_clipped_and_is_the_documented_generator():
    out = _noise_field(7, 0.0, 0.5)
    assert out.min() >= 0.0 and out.max() <= 1.0 and (out != 0.5).mean() > 0.99
    # Philox-4x32-10 + Box-Muller as include/hdf.h states them.  The device's log, sqrt and cos differ from numpy's in
    # the last bits of an fp64, 1e-16 against the 3e-8 of an fp32 step at 0.5: the rounding moves only at a tie
    want = zr.intensity_ref(np.full(NOISE_SHAPE, 0.5, np.float32), [1.0] * 4, [1] * 4, 7, 0.0)
    d = _ulps(out, want)
    print("noise: %d of %d elements one ulp from the restatement" % (int((d == 1).sum()), d.size))
    assert d.max() <= 1 and (d == 0).mean() > 0.999
    low = _intensity(np.full((1, 1, 64, 64), 0.02, np.float32), [1.0], [1], 3, 0.0)
    assert low.min() == 0.0 and (low == 0.0).mean() > 0.2                     # the lower clip bites
    neg = _intensity(np.full((1, 1, 64, 64), 0.02, np.float32), [1.0], [1], 3, -1.0)
    assert neg.min() < 0.0 and np.array_equal(neg[low > 0], low[low > 0])


def test_gamma_comes_before_the_noise():
    x = np.random.RandomState(3).uniform(0, 1, (2, 2, 17, 29)).astype(np.float32)
    got = _intensity(x, [0.8, 1.2], [1, 0], 11, 0.0)
    want = zr.intensity_ref(x, [0.8, 1.2], [1, 0], 11, 0.0)
    # the pow may sit one fp32 step (at most 2^-24 below 1) from numpy's, the sum rounds once more (2^-25): an absolute
    # bound, since the noise may carry a value near 1 down to a finer binade
    assert np.abs(got[0].astype(np.float64) - want[0]).max() <= 2.0 ** -23
    assert _ulps(got[1], zr.gamma_ref(x[1], 1.2)).max() <= 1                  # sample 1: the gamma alone
    assert np.abs(got[0] - zr.gamma_ref(x[0], 0.8)).max() > 0.1               # sample 0: the noise on top of it


def test_intensity_refusals():
    x = torch.full((2, 2, 5, 7), 0.5, device=DEV)
    g, f = np.array([0.9, 1.1]), np.array([0, 1], dtype=np.uint8)

    def call(image=x, batch=2, channels=2, h=5, w=7, gamma=g, noise=f, low=0.0):
        return lib().hdf_intensity_2d(ptr(image), batch, channels, h, w,
                                      None if gamma is None else gamma.ctypes.data_as(C.POINTER(C.c_double)),
                                      None if noise is None else noise.ctypes.data, 5, low, st())

    for what, kw in {"null image": dict(image=None), "null gamma": dict(gamma=None), "null noise": dict(noise=None),
                     "no sample": dict(batch=0), "no channel": dict(channels=0), "65 channels": dict(channels=65),
                     "zero height": dict(h=0), "too wide": dict(w=16385),
                     "negative gamma": dict(gamma=np.array([0.9, -0.1])), "NaN gamma": dict(gamma=np.array([np.nan, 1.0])),
                     "noise flag 2": dict(noise=np.array([0, 2], dtype=np.uint8)), "low_clip above 1": dict(low=1.5),
                     "NaN low_clip": dict(low=float("nan"))}.items():
        rc = call(**kw)
        assert rc != 0 and lib().hdf_last_error().startswith(b"intensity_2d:"), (what, rc, lib().hdf_last_error())
    torch.cuda.synchronize()
    assert bool((x == 0.5).all())


# --------------------------------------------------------------------------------------------------------- the chain
FULL_IDS = [1, 3, 4, 6, 7, 8, 9, 10]
CHAIN_SEEDS = (4, 8)


def _raw_batch(batch=6, shape=(48, 48)):
    rng = np.random.RandomState(21)
    image = rng.standard_normal((batch, 2) + shape).astype(np.float32)
    image[:, 0] = image[:, 0] * 300.0 + 400.0                        # MR-like range, some negatives: the clamp bites
    labels = np.stack([zr.labels_of(shape, 21 + b) % 2 for b in range(batch)]).astype(np.uint8)
    labels[0] = 0                                                    # an empty label: erase and zoom draw their windows
    labels[1] = 0
    labels[1, 40:44, 3:9] = 1                                        # a small box: the windows follow it
    return torch.tensor(image).to(DEV), torch.tensor(labels).to(DEV)


def test_full_chain_is_the_chain_of_its_parts_under_the_same_draws():
    from hdf_rt import (TrainTransform2D, augment_2d, erase2d_keep, flip2d_code, gamma2d, intensity_2d_, label_bbox_2d,
                        noise2d_flag, rotate_degree, rotate_matrix, zoom2d_canvas, zoom_2d)
    from hdf_rt.inference import mr_normalize_
    image, labels = _raw_batch()
    batch, shape = 6, (48, 48)
    keep_i, keep_l = image.clone(), labels.clone()
    tf = TrainTransform2D.from_ids(2, FULL_IDS)
    seen = {"noise": 0, "crop": 0, "pad": 0, "erase": 0}
    for seed in CHAIN_SEEDS:
        random.seed(seed), np.random.seed(seed)
        got_i, got_oh = tf(image, labels)
        assert torch.equal(image, keep_i) and torch.equal(labels, keep_l)        # the arguments are left alone
        random.seed(seed), np.random.seed(seed)
        norm = image.clone()
        mr_normalize_(norm.view(batch * 2, 1, *shape))
        bbox = label_bbox_2d(labels).cpu().numpy()
        assert np.array_equal(bbox, zr.bbox_ref(labels.cpu().numpy())) and bbox[0, 0] == 0 and bbox[1, 0] == 24
        keeps, canvases, mats, codes, gammas, flags = [], [], [], [], [], []
        for k in range(batch):                                                   # the order of the chain, per sample
            keeps.append(erase2d_keep(bbox[k], 48, 48))
            canvases.append(zoom2d_canvas(bbox[k], 48, 48))
            mats.append(rotate_matrix(rotate_degree(), 48, 48))
            codes.append(flip2d_code("hv"))
            gammas.append(gamma2d())
            flags.append(noise2d_flag())
        noise_seed = int(np.random.randint(0, 2 ** 63 - 1, dtype=np.int64))      # one per batch, after the samples
        seen["noise"] += sum(flags)
        seen["crop"] += sum(c[2] <= 0 and c[0] < 48 for c in canvases)
        seen["pad"] += sum(c[0] > 48 for c in canvases)
        seen["erase"] += sum(k != (0, 48, 0, 48) for k in keeps)
        zi, zl = zoom_2d(norm, labels, keeps, canvases)
        want_i, want_oh = augment_2d(zi, zl, 2, mats, codes)
        intensity_2d_(want_i, gammas, flags, noise_seed, 0.0)
        assert got_i.shape == (batch, 2) + shape and got_oh.shape == (batch, 2) + shape
        assert torch.equal(got_i, want_i) and torch.equal(got_oh, want_oh)
        assert bool((got_oh.sum(1) == 1).all()) and float(got_i.min()) >= 0.0
        # and the moving parts are the restatement's, bit for bit
        ref = zr.zoom2d_batch_ref(norm.cpu().numpy(), labels.cpu().numpy(), keeps, canvases)
        zr.check_exact(zi.cpu().numpy(), ref["image"], "zoom image")
        zr.check_exact(zl.cpu().numpy(), ref["labels"], "zoom labels")
    assert all(seen.values()), seen                                              # the seeds exercise every branch


def test_the_full_chain_goes_straight_into_the_2d_model_and_the_loss():
    from hdf_rt import TrainTransform2D
    from loss.combine_loss import CEPlusDice, DeepSuperloss
    from models.HDenseFormer_2D import HDenseFormer_2D
    image, labels = _raw_batch()
    shape, batch, n_cls = (48, 48), 6, 2
    random.seed(CHAIN_SEEDS[0]), np.random.seed(CHAIN_SEEDS[0])
    x, onehot = TrainTransform2D.from_ids(n_cls, FULL_IDS)(image, labels)
    for t in (x, onehot):                                            # what the model and the loss take as they are
        assert t.dtype == torch.float32 and t.is_contiguous() and t.device.type == "cuda"
        assert tuple(t.shape) == (batch, 2) + shape
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


def test_from_ids_without_training_is_the_validation_form():
    from hdf_rt import TrainTransform2D
    image, labels = _raw_batch()
    random.seed(4), np.random.seed(4)
    state, pstate = np.random.get_state()[1].copy(), random.getstate()
    got_i, got_oh = TrainTransform2D.from_ids(2, FULL_IDS, train=False)(image, labels)
    assert np.array_equal(np.random.get_state()[1], state) and random.getstate() == pstate   # no augmentation draw
    want_i, want_oh = TrainTransform2D(2, degrees=(), flip="")(image, labels)
    assert torch.equal(got_i, want_i) and torch.equal(got_oh, want_oh)
    # and the default list is today's default chain
    random.seed(4), np.random.seed(4)
    a_i, a_oh = TrainTransform2D.from_ids(2, [1, 6, 7, 10])(image, labels)
    random.seed(4), np.random.seed(4)
    b_i, b_oh = TrainTransform2D(2)(image, labels)
    assert torch.equal(a_i, b_i) and torch.equal(a_oh, b_oh)
