"""The reference's 3-D training transform chain on the device (trainer.py:128-146 with config.py's
transform_3d = [1,2,4,5,6]): RandomCrop3D is a slice, PETandCTNormalize / MRNormalize the in-place kernels of
hdf_rt.inference, and RandomTranslationRotationZoom3D + RandomFlip3D + To_Tensor ONE gather kernel per sample
(hdf_augment_3d, csrc/augment.hip).  The random draws stay on the host and follow the reference's order, so seeding
np.random / random reproduces its parameters.  No CPU fallback.

The other 3-D chain, transform_3d = [2,3,4,5,6] (config.py:116): the whole volume is normalised, CropResize (3) brings it to
input_shape -- resize_3d / crop_resize, skimage's anti-aliased resize as at most three separable gather passes per plane
(hdf_resize_3d, csrc/resize.hip) -- and the warp, flip and one-hot follow.  Trunc_and_Normalize (7) is trunc_normalize_.
TrainTransform3D.from_ids maps the reference's ids 1..8.

The default 2-D chain (trainer.py:152-172 with config.py's transform_2d = [1,6,7,10]): MRNormalize per plane, then
RandomRotate2D + RandomFlip2D + To_Tensor ONE gather kernel per batch (hdf_augment_2d), bit for bit what PIL computes
on the host (pinned to PIL 12.2.0; include/hdf.h).  The matrix is built here, in Python, because PIL rounds the cosine
and the sine with Python's decimal round(., 15).

The rest of the 2-D list (trainer.py:152-168): RandomErase2D (3) and RandomZoom2D (4) are one gather launch before the
rotation (hdf_zoom_2d, bit for bit PIL's crop / ImageOps.expand + resize), fed by one label bounding-box reduction per
batch (hdf_label_bbox_2d); RandomAdjust2D (8) and RandomNoise2D (9) one in-place launch after it (hdf_intensity_2d).
TrainTransform2D.from_ids maps the reference's ids; CropResize (2), RandomDistort2D (5) and Trunc_and_Normalize (11) are
refused by name."""
import ctypes as C
import math
import random

import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr, stream_ptr
from .inference import mr_normalize_, onehot_from_labels, pet_ct_normalize_


def trz_matrix(mode="tr", rng=np.random):
    """[A | t] of RandomTranslationRotationZoom3D (data_utils/transformer_3d.py:73-99) as a (3, 4) float64 array,
    drawing from `rng` in the reference's order: translation (0, U(-5,5), U(-5,5)) if 't', the angle U(-5,5) degrees
    about axis 0 if 'r', zoom (1, U(.9,1.1), U(.9,1.1)) if 'z'.  compose(T, R, Z) = [R diag(Z) | T] and
    euler2mat(a, 0, 0, 'sxyz') = [[1,0,0],[0,cos a,-sin a],[0,sin a,cos a]] in closed form."""
    t = [0.0, rng.uniform(-5, 5), rng.uniform(-5, 5)] if "t" in mode else [0.0, 0.0, 0.0]
    a = rng.uniform(-5, 5) / 180.0 * np.pi if "r" in mode else 0.0
    z = [1.0, rng.uniform(0.9, 1.1), rng.uniform(0.9, 1.1)] if "z" in mode else [1.0, 1.0, 1.0]
    ca, sa = math.cos(a), math.sin(a)
    rot = np.array([[1.0, 0.0, 0.0], [0.0, ca, -sa], [0.0, sa, ca]], dtype=np.float64)
    out = np.empty((3, 4), dtype=np.float64)
    out[:, :3] = rot * np.asarray(z, dtype=np.float64)[None, :]
    out[:, 3] = t
    return out


def flip_flags(mode="hv", rng=np.random):
    """(flip_h, flip_w) of RandomFlip3D (data_utils/transformer_3d.py:143-163): 'hv' draws one U(0,1) and flips H when
    it exceeds 0.5, else W -- one flip always happens; 'h' or 'v' alone flips that axis without a draw; '' none."""
    if "h" in mode and "v" in mode:
        h = bool(rng.uniform(0, 1) > 0.5)
        return h, not h
    return "h" in mode, "v" in mode


def crop_origin(shape, patch, rng=random):
    """Origins of RandomCrop3D (data_utils/transformer_3d.py:18-20): on every axis longer than the patch
    rng.randint(0, size - patch), both ends included, drawn in axis order; 0 elsewhere."""
    return tuple(rng.randint(0, int(s) - int(p)) if int(s) > int(p) else 0 for s, p in zip(shape, patch))


def augment_3d(image, labels, n_cls, affine, flip_h=False, flip_w=False, out_image=None, out_onehot=None,
               out_labels=None):
    """Warp + flip + one-hot of one sample in one launch.  image: fp32 device tensor [C, D, H, W]; labels: uint8 device
    tensor [D, H, W] (None: image only); affine: (3, 4) float64 from trz_matrix.  Returns (image, onehot): new tensors,
    or out_image [C, D, H, W] / out_onehot [n_cls, D, H, W] when given -- contiguous slices of batch tensors, so a
    batch loop writes in place.  out_labels (uint8 [D, H, W]) also receives the warped class map.  Semantics:
    include/hdf.h, hdf_augment_3d."""
    if not torch.is_tensor(image) or image.device.type != "cuda":
        raise _lib.HdfError("augment_3d needs device tensors (there is no CPU path)")
    if image.dtype != torch.float32 or image.dim() != 4:
        raise ValueError(f"image must be a float32 tensor [C, D, H, W], got {image.dtype} {tuple(image.shape)}")
    image = image.contiguous()
    c, vol = int(image.shape[0]), tuple(int(s) for s in image.shape[1:])
    if labels is not None:
        if (not torch.is_tensor(labels) or labels.device != image.device or labels.dtype != torch.uint8
                or tuple(labels.shape) != vol):
            raise ValueError(f"labels must be a uint8 tensor {vol} on {image.device}")
        labels = labels.contiguous()
    aff = np.ascontiguousarray(affine, dtype=np.float64)
    if aff.shape != (3, 4):
        raise ValueError(f"affine must be (3, 4), got {aff.shape}")

    def out(t, shape, dtype, what):
        if t is None:
            return torch.empty(shape, dtype=dtype, device=image.device)
        if (not torch.is_tensor(t) or t.device != image.device or t.dtype != dtype or tuple(t.shape) != shape
                or not t.is_contiguous()):
            raise ValueError(f"{what} must be a contiguous {dtype} tensor {shape} on {image.device}")
        return t

    out_image = out(out_image, (c,) + vol, torch.float32, "out_image")
    if labels is None:
        if out_onehot is not None or out_labels is not None:
            raise ValueError("a label output needs labels")
    else:
        out_onehot = out(out_onehot, (n_cls,) + vol, torch.float32, "out_onehot")
        if out_labels is not None:
            out(out_labels, vol, torch.uint8, "out_labels")
    check(lib().hdf_augment_3d(ptr(image), ptr(labels), c, n_cls, vol[0], vol[1], vol[2],
                               aff.ctypes.data_as(C.POINTER(C.c_double)), int(bool(flip_h)), int(bool(flip_w)),
                               ptr(out_image), ptr(out_labels), ptr(out_onehot), stream_ptr()), "hdf_augment_3d")
    return out_image, out_onehot


_RESIZE_WS = {}      # (device, source shape, result shape) -> the fp64 intermediates of one plane
_RESIZE_WS_KEEP = 8  # shapes kept, the most recently used last: a dataset of many volume sizes does not pile them up


def _shape3(shape, what):
    try:
        out = tuple(int(v) for v in shape)
    except TypeError:
        out = ()
    if len(out) != 3 or any(int(v) != v for v in shape):
        raise ValueError(f"{what} must be three integers (D, H, W), got {shape!r}")
    return out


def resize_3d(image, labels, n_cls, out_shape, out_image=None, out_labels=None):
    """The resize of CropResize (data_utils/data_loader.py:103-119) of one sample: image fp32 device tensor [C, D, H, W]
    -> [C, *out_shape], each channel skimage.transform.resize(., out_shape, anti_aliasing=True); labels uint8 device
    tensor [D, H, W] -> uint8 [*out_shape], the per-class resize(mode='constant') >= 0.5 with the last class winning.
    Either may be None.  Returns (image, labels): new tensors, or out_image / out_labels when given.  The fp64
    intermediates of one plane live in a workspace cached per (device, shapes), the last few shapes kept.  Semantics:
    include/hdf.h, hdf_resize_3d."""
    first = image if image is not None else labels
    if first is None:
        raise ValueError("resize_3d needs an image, labels or both")
    if not torch.is_tensor(first) or first.device.type != "cuda":
        raise _lib.HdfError("resize_3d needs device tensors (there is no CPU path)")
    dev = first.device
    dst = _shape3(out_shape, "out_shape")
    c = 0
    if image is not None:
        if image.dtype != torch.float32 or image.dim() != 4:
            raise ValueError(f"image must be a float32 tensor [C, D, H, W], got {image.dtype} {tuple(image.shape)}")
        image = image.contiguous()
        c, src = int(image.shape[0]), tuple(int(v) for v in image.shape[1:])
    if labels is not None:
        if (not torch.is_tensor(labels) or labels.device != dev or labels.dtype != torch.uint8 or labels.dim() != 3
                or (image is not None and tuple(labels.shape) != src)):
            raise ValueError(f"labels must be a uint8 tensor {src if image is not None else '[D, H, W]'} on {dev}")
        labels = labels.contiguous()
        src = tuple(int(v) for v in labels.shape)

    def out(t, shape, dtype, what):
        if t is None:
            return torch.empty(shape, dtype=dtype, device=dev)
        if (not torch.is_tensor(t) or t.device != dev or t.dtype != dtype or tuple(t.shape) != shape
                or not t.is_contiguous()):
            raise ValueError(f"{what} must be a contiguous {dtype} tensor {shape} on {dev}")
        return t

    if image is None and out_image is not None:
        raise ValueError("out_image needs an image")
    if labels is None and out_labels is not None:
        raise ValueError("out_labels needs labels")
    if image is not None:
        out_image = out(out_image, (c,) + dst, torch.float32, "out_image")
    if labels is not None:
        out_labels = out(out_labels, dst, torch.uint8, "out_labels")
    nbytes = int(lib().hdf_resize_workspace_bytes(*src, *dst))
    if nbytes < 0:
        raise ValueError(f"resize_3d: {src} -> {dst} is outside the kernel's limits: every dimension 1..1024, no axis "
                         f"shrinking by more than a factor of 8")
    key = (dev, src, dst)
    ws = _RESIZE_WS.pop(key, None)
    if ws is None:
        ws = torch.empty(max(nbytes // 8, 1), dtype=torch.float64, device=dev)
    _RESIZE_WS[key] = ws
    while len(_RESIZE_WS) > _RESIZE_WS_KEEP:
        del _RESIZE_WS[next(iter(_RESIZE_WS))]
    check(lib().hdf_resize_3d(ptr(image), ptr(labels), c, n_cls, *src, *dst, ptr(out_image), ptr(out_labels), ptr(ws),
                              nbytes, stream_ptr()), "hdf_resize_3d")
    return out_image, out_labels


def crop_resize(image, labels, n_cls, dim, crop=0):
    """CropResize.__call__ (data_utils/data_loader.py:85-123) on device tensors: with crop != 0 image and labels become
    [..., crop:-crop, crop:-crop] -- the last two axes only --, then resize_3d to `dim` when labels.shape != dim.  A 2-D
    sample (image [C, H, W], labels [H, W], dim of two) goes through as [C, 1, H, W] / [1, H, W].  Returns (image,
    labels); without a resize they are the (sliced) arguments themselves, as in the reference."""
    if not torch.is_tensor(image) or image.device.type != "cuda":
        raise _lib.HdfError("crop_resize needs device tensors (there is no CPU path)")
    crop = int(crop)
    if crop != 0:
        image = image[..., crop:-crop, crop:-crop]
        labels = labels[..., crop:-crop, crop:-crop]
    if dim is None or tuple(labels.shape) == tuple(int(v) for v in dim):
        return image, labels
    if labels.dim() == 2:
        if len(dim) != 2 or image.dim() != 3:
            raise ValueError(f"a 2-D sample is image [C, H, W], labels [H, W] and dim (H, W), got {tuple(image.shape)}, "
                             f"{tuple(labels.shape)} and {dim!r}")
        out_i, out_l = resize_3d(image[:, None], labels[None], n_cls, (1,) + tuple(dim))
        return out_i[:, 0], out_l[0]
    return resize_3d(image, labels, n_cls, dim)


def trunc_normalize_(image, scale):
    """Trunc_and_Normalize(scale) (data_utils/data_loader.py:16-36) in place on an fp32 device tensor of any shape:
    ((x - scale[0]) clamped to [0, scale[1] - scale[0]]) / (scale[1] - scale[0]), bit for bit numpy's fp32 sequence.
    Returns image."""
    if not torch.is_tensor(image) or image.device.type != "cuda":
        raise _lib.HdfError("trunc_normalize_ needs a device tensor (there is no CPU path)")
    if image.dtype != torch.float32 or not image.is_contiguous():
        raise ValueError(f"image must be a contiguous float32 tensor, got {image.dtype} with strides {image.stride()}")
    if scale is None or len(scale) != 2:
        raise ValueError(f"scale must be a pair (lo, hi), got {scale!r}")
    check(lib().hdf_trunc_normalize(ptr(image), image.numel(), float(scale[0]), float(scale[1]), stream_ptr()),
          "hdf_trunc_normalize")
    return image


# the reference's transform_list_3d (trainer.py:128-142) by id
TRANSFORM_3D_NAMES = {1: "RandomCrop3D", 2: "PETandCTNormalize", 3: "CropResize", 4: "RandomTranslationRotationZoom3D",
                      5: "RandomFlip3D", 6: "To_Tensor", 7: "Trunc_and_Normalize", 8: "MRNormalize"}
# the orders from_ids accepts: the subsequences of this list of slots
_SLOTS_3D = ((1,), (2, 7, 8), (3,), (4,), (5,), (6,), (7,))
_ORDER_3D = "1, one of 2 | 7 | 8, 3, 4, 5, 6, 7"


class TrainTransform3D:
    """transform_3d = [1,2,4,5,6] (normalize='petct') or [1,8,4,5,6] ('mr') of trainer.py:128-146 on device tensors:
    RandomCrop3D -> normalisation -> RandomTranslationRotationZoom3D(mode) -> RandomFlip3D(flip) -> To_Tensor.
    mode='' and flip='' give the validation chain (trainer.py:147-150: crop, normalise, one-hot).  The crop comes before
    the warp, so the warp's zero border is the border of the crop.

    Off unless asked for, by keyword: resize=dim with crop runs CropResize(dim, crop=crop) between the normalisation and
    the warp ([2,3,4,5,6] of config.py:116: the WHOLE volume is normalised and resized to dim, which draws nothing);
    normalize='trunc' with scale=(lo, hi) is Trunc_and_Normalize as the normaliser ([1,7,4,5,6]); trunc_after=True
    applies it to the image after the one-hot ([...,6,7]).  from_ids maps the reference's ids."""

    def __init__(self, n_cls, patch_size=None, normalize=None, mode="tr", flip="hv", *, resize=None, crop=0, scale=None,
                 trunc_after=False):
        if normalize not in (None, "petct", "mr", "trunc"):
            raise ValueError(f"normalize must be None, 'petct', 'mr' or 'trunc', got {normalize!r}")
        if (normalize == "trunc" or trunc_after) and (scale is None or len(scale) != 2 or not scale[1] > scale[0]):
            raise ValueError(f"Trunc_and_Normalize needs scale=(lo, hi) with hi > lo, got {scale!r}")
        if resize is not None:
            resize = _shape3(resize, "resize")
        if int(crop) < 0 or (crop and resize is None):
            raise ValueError(f"crop={crop!r}: a non-negative margin of CropResize, which needs resize=dim")
        self.n_cls, self.patch_size, self.normalize, self.mode, self.flip = n_cls, patch_size, normalize, mode, flip
        self.resize, self.crop, self.trunc_after = resize, int(crop), bool(trunc_after)
        self.scale = None if scale is None else (scale[0], scale[1])

    @classmethod
    def from_ids(cls, n_cls, transform_3d, input_shape=None, patch_size=None, crop=0, scale=None, train=True):
        """The chain the reference builds from config.py's transform_3d (trainer.py:128-150): ids into its list, run in
        the order given.  1 RandomCrop3D(patch_size), 2 PETandCTNormalize, 3 CropResize(input_shape, crop), 4
        RandomTranslationRotationZoom3D('tr'), 5 RandomFlip3D('hv'), 6 To_Tensor, 7 Trunc_and_Normalize(scale), 8
        MRNormalize.  Accepted orders: the subsequences of 1, one of 2 | 7 | 8, 3, 4, 5, 6, 7 (a 7 before the one-hot is
        the normaliser, one after it rescales the finished image); anything else raises ValueError.  6 must be present:
        the chain returns the one-hot.  train=False keeps ids 1, 2, 3 and 6 only, as trainer.py:147-150 does -- which
        drops the normalisers 7 and 8 from the validation chain; the quirk is kept."""
        ids = [int(i) for i in transform_3d]
        for i in ids:
            if i not in TRANSFORM_3D_NAMES:
                raise ValueError(f"transform_3d id {i} is not in the reference's list (1..8)")
        if not train:
            ids = [i for i in ids if i in (1, 2, 3, 6)]
        slot, taken = 0, {}
        for i in ids:
            while slot < len(_SLOTS_3D) and i not in _SLOTS_3D[slot]:
                slot += 1
            if slot == len(_SLOTS_3D):
                raise ValueError(f"transform_3d {ids} does not run on the device: the accepted order is a subsequence of "
                                 f"{_ORDER_3D}")
            taken[slot] = i
            slot += 1
        if 5 not in taken:
            raise ValueError("transform_3d must hold 6 (To_Tensor): the chain returns the one-hot")
        if 0 in taken and patch_size is None:
            raise ValueError("transform_3d id 1 (RandomCrop3D) needs patch_size")
        if 2 in taken and input_shape is None:
            raise ValueError("transform_3d id 3 (CropResize) needs input_shape")
        return cls(n_cls, patch_size=patch_size if 0 in taken else None,
                   normalize={None: None, 2: "petct", 7: "trunc", 8: "mr"}[taken.get(1)],
                   mode="tr" if 3 in taken else "", flip="hv" if 4 in taken else "",
                   resize=input_shape if 2 in taken else None, crop=crop if 2 in taken else 0,
                   scale=scale if (taken.get(1) == 7 or 6 in taken) else None, trunc_after=6 in taken)

    def draw(self, shape):
        """The random parameters of one sample whose labels have `shape`, drawn in the reference's order and nothing
        else: the crop origin (random; None without a patch), the warp's matrix (np.random) and the flip flags
        (np.random).  The resize and the normalisers draw nothing."""
        origin = None
        if self.patch_size is not None:
            origin = crop_origin(shape, tuple(int(v) for v in self.patch_size))
        return origin, trz_matrix(self.mode), flip_flags(self.flip)

    def __call__(self, image, labels):
        """image: raw fp32 [C, Ds, Hs, Ws], labels: uint8 [Ds, Hs, Ws], both on the device.  Returns (image [C, D, H, W],
        onehot [n_cls, D, H, W]); the arguments are left untouched."""
        if not torch.is_tensor(image) or image.device.type != "cuda":
            raise _lib.HdfError("TrainTransform3D needs device tensors (there is no CPU path)")
        o, affine, flips = self.draw(labels.shape)
        if o is not None:
            p = tuple(int(v) for v in self.patch_size)
            image = image[:, o[0]:o[0] + p[0], o[1]:o[1] + p[1], o[2]:o[2] + p[2]]
            labels = labels[o[0]:o[0] + p[0], o[1]:o[1] + p[1], o[2]:o[2] + p[2]]
        image = image.clone(memory_format=torch.contiguous_format)     # the normalisation works in place
        labels = labels.contiguous()
        if self.normalize == "petct":
            pet_ct_normalize_(image)
        elif self.normalize == "mr":
            mr_normalize_(image)
        elif self.normalize == "trunc":
            trunc_normalize_(image, self.scale)
        if self.resize is not None:
            image, labels = crop_resize(image, labels, self.n_cls, self.resize, self.crop)
            image, labels = image.contiguous(), labels.contiguous()
        if not self.mode and not self.flip:
            image, onehot = image, onehot_from_labels(labels[None], self.n_cls)[0]
        else:
            image, onehot = augment_3d(image, labels, self.n_cls, affine, *flips)
        if self.trunc_after:
            trunc_normalize_(image, self.scale)
        return image, onehot


# ---------------------------------------------------------------------------------------------------------- 2-D chain
REFERENCE_DEGREES = (-15, -10, -5, 0, 5, 10, 15)        # RandomRotate2D's default (data_utils/transformer_2d.py:144)


def rotate_matrix(angle, width, height):
    """The six doubles (a, b, c, d, e, f) PIL's Image.rotate(angle) hands to Image.transform(AFFINE) for a width x
    height image: output pixel -> input coordinate, about the centre (width / 2, height / 2), the cosine and sine
    rounded with Python's round(., 15) as PIL does.  PIL short-cuts 0, 180 and square 90 / 270 degrees to copies and
    transposes; this general form gives the same bits there (tests/test_augment2d_ref_cpu.py)."""
    ang = -math.radians(angle % 360)
    cx, cy = width / 2.0, height / 2.0
    a, b = round(math.cos(ang), 15), round(math.sin(ang), 15)
    d, e = round(-math.sin(ang), 15), round(math.cos(ang), 15)
    c = (a * (-cx) + b * (-cy) + 0.0) + cx
    f = (d * (-cx) + e * (-cy) + 0.0) + cy
    return (a, b, c, d, e, f)


def rotate_degree(degrees=REFERENCE_DEGREES, rng=random):
    """The angle of RandomRotate2D (data_utils/transformer_2d.py:161): rng.choice of the list."""
    return rng.choice(list(degrees))


def flip2d_code(mode="hv", rng=np.random):
    """The flip of RandomFlip2D (data_utils/transformer_2d.py:99-128) as hdf_augment_2d's code, 0 none, 1 mirrors W,
    2 mirrors H.  'hv': one U(0,1); below 0.3 gives 1, below 0.6 gives 2, else 0 (never both).  'h' alone: one draw,
    above 0.5 gives 1; 'v' alone: one draw, above 0.5 gives 2; '': no draw, 0."""
    if "h" in mode and "v" in mode:
        u = rng.uniform(0, 1)
        return 1 if u < 0.3 else 2 if u < 0.6 else 0
    if "h" in mode:
        return 1 if rng.uniform(0, 1) > 0.5 else 0
    if "v" in mode:
        return 2 if rng.uniform(0, 1) > 0.5 else 0
    return 0


def augment_2d(image, labels, n_cls, matrices, flips, out_image=None, out_onehot=None, out_labels=None):
    """Rotation + flip + one-hot of a batch in one launch per 32 samples.  image: fp32 device tensor [B, C, H, W];
    labels: uint8 device tensor [B, H, W] (None: image only); matrices: [B][6] doubles from rotate_matrix; flips: [B]
    codes from flip2d_code.  Returns (image, onehot): new tensors, or out_image [B, C, H, W] / out_onehot
    [B, n_cls, H, W] when given; out_labels (uint8 [B, H, W]) also receives the moved class map.  Semantics:
    include/hdf.h, hdf_augment_2d."""
    if not torch.is_tensor(image) or image.device.type != "cuda":
        raise _lib.HdfError("augment_2d needs device tensors (there is no CPU path)")
    if image.dtype != torch.float32 or image.dim() != 4:
        raise ValueError(f"image must be a float32 tensor [B, C, H, W], got {image.dtype} {tuple(image.shape)}")
    image = image.contiguous()
    b, c, h, w = (int(s) for s in image.shape)
    if labels is not None:
        if (not torch.is_tensor(labels) or labels.device != image.device or labels.dtype != torch.uint8
                or tuple(labels.shape) != (b, h, w)):
            raise ValueError(f"labels must be a uint8 tensor {(b, h, w)} on {image.device}")
        labels = labels.contiguous()
    mats = np.ascontiguousarray(matrices, dtype=np.float64)
    if mats.shape != (b, 6):
        raise ValueError(f"matrices must be ({b}, 6), got {mats.shape}")
    codes = np.asarray(flips)
    if codes.shape != (b,) or codes.dtype.kind not in "iub" or ((codes < 0) | (codes > 2)).any():
        raise ValueError(f"flips must be {b} codes in (0, 1, 2), got {flips!r}")
    codes = np.ascontiguousarray(codes, dtype=np.uint8)

    def out(t, shape, dtype, what):
        if t is None:
            return torch.empty(shape, dtype=dtype, device=image.device)
        if (not torch.is_tensor(t) or t.device != image.device or t.dtype != dtype or tuple(t.shape) != shape
                or not t.is_contiguous()):
            raise ValueError(f"{what} must be a contiguous {dtype} tensor {shape} on {image.device}")
        return t

    out_image = out(out_image, (b, c, h, w), torch.float32, "out_image")
    if labels is None:
        if out_onehot is not None or out_labels is not None:
            raise ValueError("a label output needs labels")
    else:
        out_onehot = out(out_onehot, (b, n_cls, h, w), torch.float32, "out_onehot")
        if out_labels is not None:
            out(out_labels, (b, h, w), torch.uint8, "out_labels")
    check(lib().hdf_augment_2d(ptr(image), ptr(labels), b, c, n_cls, h, w, mats.ctypes.data_as(C.POINTER(C.c_double)),
                               codes.ctypes.data, ptr(out_image), ptr(out_labels), ptr(out_onehot), stream_ptr()),
          "hdf_augment_2d")
    return out_image, out_onehot


# --------------------------------------------------------------------------------- erase, zoom, gamma, noise (2-D)
def erase2d_keep(bbox_row, H, W, window=(64, 64), rng=random):
    """The keep-rectangle (r0, r1, c0, c1) of RandomErase2D(scale_flag=False) (data_utils/transformer_2d.py:32-73) for a
    sample whose label bounding box is bbox_row = (nonzero_count, rmin, rmax, cmin, cmax), drawing from `rng` in the
    reference's order.  Non-empty label: the window is the box grown by half of `window`, clamped to the plane, no draw;
    empty label: four rng.randint, (0, 64), (-64, 0) for the rows, then the same for the columns (the reference's
    literals).  Then rng.choice of the direction: 't' zeroes rows [:rw0[0]], 'd' rows [rw0[1]:], 'l' columns [:rw1[0]],
    'r' columns [rw1[1]:], 'no_erase' nothing -- with Python's slice rules, so a drawn 0 for 'd' or 'r' erases the whole
    plane and a negative value counts from the end."""
    n, rmin, rmax, cmin, cmax = (int(v) for v in bbox_row)
    max_h, max_w = window
    if n != 0:
        rw0 = (max(rmin - max_h // 2, 0), min(rmax + max_h // 2, H))
        rw1 = (max(cmin - max_w // 2, 0), min(cmax + max_w // 2, W))
    else:
        rw0 = (rng.randint(0, 64), rng.randint(-64, 0))
        rw1 = (rng.randint(0, 64), rng.randint(-64, 0))
    direction = rng.choice(['t', 'd', 'l', 'r', 'no_erase'])
    r0, r1, c0, c1 = 0, H, 0, W
    if direction == 't':
        r0 = slice(None, rw0[0]).indices(H)[1]
    elif direction == 'd':
        r1 = slice(rw0[1], None).indices(H)[0]
    elif direction == 'l':
        c0 = slice(None, rw1[0]).indices(W)[1]
    elif direction == 'r':
        c1 = slice(rw1[1], None).indices(W)[0]
    return (r0, r1, c0, c1)


def zoom2d_canvas(bbox_row, H, W, scale=(0.8, 1.2), rng=random):
    """The canvas (sw, sh, ox, oy) of RandomZoom2D (data_utils/transformer_2d.py:207-259) for hdf_zoom_2d, drawing from
    `rng` in the reference's order: s = rng.uniform(*scale), tw = int(W * s), th = int(H * s).
    s < 1, a crop at (x1, y1): an empty label draws x1 = randint(0, W - th), y1 = randint(0, H - tw) -- the reference
    reads PIL's (width, height) as (h, w), so th bounds the column and tw the row; the swap is kept.  A non-empty one,
    with xl = max(0, rmin), xr = min(H, rmax), yl = max(0, cmin), yr = min(W, cmax): x1 = randint(max(0, min(yl, yr -
    th)), min(yl, W - th)), then y1 = randint(max(0, min(xl, xr - tw)), min(xl, H - tw)).  An empty range raises
    ValueError, as random.randint does in the reference.  The canvas is (tw, th, -x1, -y1).
    s >= 1, a pad: p0 = int(rng.uniform(0, (tw - H) / 2)), p1 = int(rng.uniform(0, (th - W) / 2)), then
    ImageOps.expand(border=(p0, p1, tw - H, th - W)) -- the same swap: the reference's `tw - w` and `th - h` subtract the
    height from the padded width and the width from the padded height.  The canvas is (p0 + W + tw - H, p1 + H + th - W,
    p0, p1); on a square plane, the reference's own case, that is (tw + p0, th + p1, p0, p1) with p0 below (tw - W) / 2."""
    n, rmin, rmax, cmin, cmax = (int(v) for v in bbox_row)
    s = rng.uniform(scale[0], scale[1])
    tw, th = int(W * s), int(H * s)
    if s < 1.:
        if n == 0:
            cols, rows = (0, W - th), (0, H - tw)
        else:
            xl, xr, yl, yr = max(0, rmin), min(H, rmax), max(0, cmin), min(W, cmax)
            rows = (max(0, min(xl, xr - tw)), min(xl, H - tw))
            cols = (max(0, min(yl, yr - th)), min(yl, W - th))
        x1 = rng.randint(cols[0], cols[1])
        y1 = rng.randint(rows[0], rows[1])
        return (tw, th, -x1, -y1)
    p0 = int(rng.uniform(0, (tw - H) / 2))
    p1 = int(rng.uniform(0, (th - W) / 2))
    return (p0 + W + tw - H, p1 + H + th - W, p0, p1)


def gamma2d(scale=(0.8, 1.2), rng=random):
    """The gamma of RandomAdjust2D (data_utils/transformer_2d.py:297): one rng.uniform."""
    return rng.uniform(scale[0], scale[1])


def noise2d_flag(rng=random):
    """RandomNoise2D (data_utils/transformer_2d.py:317-318): one rng.uniform(0, 1); the noise is on above 0.9."""
    return rng.uniform(0, 1) > 0.9


def _device_batch(image, what):
    if not torch.is_tensor(image) or image.device.type != "cuda":
        raise _lib.HdfError(f"{what} needs device tensors (there is no CPU path)")


def _int_rows(rows, b, what):
    a = np.asarray(rows)
    if a.shape != (b, 4) or a.dtype.kind not in "iu":
        raise ValueError(f"{what} must be ({b}, 4) integers, got {rows!r}")
    return np.ascontiguousarray(a, dtype=np.int32)


def label_bbox_2d(labels):
    """(nonzero_count, rmin, rmax, cmin, cmax) of every class map of a uint8 device batch [B, H, W] as an int32 device
    tensor [B, 5]; (0, H, -1, W, -1) for an empty one.  Semantics: include/hdf.h, hdf_label_bbox_2d."""
    _device_batch(labels, "label_bbox_2d")
    if labels.dtype != torch.uint8 or labels.dim() != 3:
        raise ValueError(f"labels must be a uint8 tensor [B, H, W], got {labels.dtype} {tuple(labels.shape)}")
    labels = labels.contiguous()
    b, h, w = (int(s) for s in labels.shape)
    nbytes = int(lib().hdf_label_bbox_workspace_bytes(b))
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=labels.device)
    out = torch.empty((b, 5), dtype=torch.int32, device=labels.device)
    check(lib().hdf_label_bbox_2d(ptr(labels), b, h, w, ptr(out), ptr(ws), nbytes, stream_ptr()), "hdf_label_bbox_2d")
    return out


def zoom_2d(image, labels, keeps, canvases, out_image=None, out_labels=None):
    """Erase + crop or pad + resample of a batch in one launch per 32 samples.  image: fp32 device tensor [B, C, H, W];
    labels: uint8 device tensor [B, H, W] (None: image only); keeps: [B][4] from erase2d_keep ((0, H, 0, W) erases
    nothing); canvases: [B][4] from zoom2d_canvas ((W, H, 0, 0) zooms nothing).  Returns (image, labels): new tensors, or
    out_image / out_labels when given.  Semantics: include/hdf.h, hdf_zoom_2d."""
    _device_batch(image, "zoom_2d")
    if image.dtype != torch.float32 or image.dim() != 4:
        raise ValueError(f"image must be a float32 tensor [B, C, H, W], got {image.dtype} {tuple(image.shape)}")
    image = image.contiguous()
    b, c, h, w = (int(s) for s in image.shape)
    if labels is not None:
        if (not torch.is_tensor(labels) or labels.device != image.device or labels.dtype != torch.uint8
                or tuple(labels.shape) != (b, h, w)):
            raise ValueError(f"labels must be a uint8 tensor {(b, h, w)} on {image.device}")
        labels = labels.contiguous()
    keep, canvas = _int_rows(keeps, b, "keeps"), _int_rows(canvases, b, "canvases")

    def out(t, shape, dtype, what):
        if t is None:
            return torch.empty(shape, dtype=dtype, device=image.device)
        if (not torch.is_tensor(t) or t.device != image.device or t.dtype != dtype or tuple(t.shape) != shape
                or not t.is_contiguous()):
            raise ValueError(f"{what} must be a contiguous {dtype} tensor {shape} on {image.device}")
        return t

    out_image = out(out_image, (b, c, h, w), torch.float32, "out_image")
    if labels is None:
        if out_labels is not None:
            raise ValueError("a label output needs labels")
    else:
        out_labels = out(out_labels, (b, h, w), torch.uint8, "out_labels")
    check(lib().hdf_zoom_2d(ptr(image), ptr(labels), b, c, h, w, keep.ctypes.data, canvas.ctypes.data, ptr(out_image),
                            ptr(out_labels), stream_ptr()), "hdf_zoom_2d")
    return out_image, out_labels


def intensity_2d_(image, gammas, noise, seed=0, low_clip=0.0):
    """Gamma and Gaussian noise in place on an fp32 device batch [B, C, H, W], one launch per 32 samples.  gammas: [B]
    from gamma2d (1.0 leaves a sample alone); noise: [B] flags from noise2d_flag; seed: the 64-bit key of the noise
    field; low_clip: 0 for an image without negatives (after MRNormalize), -1 otherwise, as skimage chooses.  Returns
    image.  Semantics: include/hdf.h, hdf_intensity_2d."""
    _device_batch(image, "intensity_2d_")
    if image.dtype != torch.float32 or image.dim() != 4 or not image.is_contiguous():
        raise ValueError(f"image must be a contiguous float32 tensor [B, C, H, W], got {image.dtype} "
                         f"{tuple(image.shape)}")
    b, c, h, w = (int(s) for s in image.shape)
    g = np.ascontiguousarray(gammas, dtype=np.float64)
    flags = np.ascontiguousarray(np.asarray(noise), dtype=np.uint8)
    if g.shape != (b,) or flags.shape != (b,):
        raise ValueError(f"gammas and noise must hold {b} values each, got {g.shape} and {flags.shape}")
    check(lib().hdf_intensity_2d(ptr(image), b, c, h, w, g.ctypes.data_as(C.POINTER(C.c_double)), flags.ctypes.data,
                                 int(seed) & (2 ** 64 - 1), float(low_clip), stream_ptr()), "hdf_intensity_2d")
    return image


# the reference's transform_list_2d (trainer.py:152-168) by id
TRANSFORM_2D_NAMES = {1: "MRNormalize", 2: "CropResize", 3: "RandomErase2D", 4: "RandomZoom2D", 5: "RandomDistort2D",
                      6: "RandomRotate2D", 7: "RandomFlip2D", 8: "RandomAdjust2D", 9: "RandomNoise2D", 10: "To_Tensor",
                      11: "Trunc_and_Normalize"}
_REFUSED_2D = {2: "it needs skimage's anti-aliased resize, for which no exact contract is pinned",
               5: "it is OpenCV's GaussianBlur + resize + fixed-point remap, for which no exact contract is pinned",
               11: "it is not part of the device chain"}


class TrainTransform2D:
    """transform_2d = [1,6,7,10] of trainer.py:152-172 on a device batch: MRNormalize (normalize='mr') ->
    RandomRotate2D(degrees) -> RandomFlip2D(flip) -> To_Tensor.  degrees=() and flip='' give the validation chain
    (trainer.py:173-176: normalise, one-hot).  MRNormalize works per plane, so a batch is simply more channels.

    The other entries of the list are off unless asked for: erase=(64, 64) is RandomErase2D(scale_flag=False) with that
    window, zoom=(0.8, 1.2) RandomZoom2D, gamma=(0.8, 1.2) RandomAdjust2D, noise=True RandomNoise2D; from_ids maps the
    reference's ids.  The order is the list's: normalise, erase, zoom, rotate, flip, gamma, noise, one-hot.  Erase, zoom,
    rotation and flip are exact to the reference's PIL calls; the gamma is pow in fp64 rounded once (the reference's is
    numpy's fp32 power); the noise is statistical: N(0, 0.01) from a counter-based generator keyed by ONE
    np.random.randint per batch, where the reference draws C*H*W normals per noisy sample from np.random -- the one
    place where the np.random stream leaves the reference's.  Noise needs normalize='mr': skimage clips at 0 when the
    image holds no negative, which MRNormalize guarantees without a reduction."""

    def __init__(self, n_cls, normalize="mr", degrees=REFERENCE_DEGREES, flip="hv", erase=None, zoom=None, gamma=None,
                 noise=False):
        if normalize not in (None, "mr"):
            raise ValueError(f"normalize must be None or 'mr', got {normalize!r}")
        if noise and normalize != "mr":
            raise ValueError("noise needs normalize='mr': its lower clip is 0 only for an image without negatives")
        for name, pair in (("erase", erase), ("zoom", zoom), ("gamma", gamma)):
            if pair is not None and (not isinstance(pair, tuple) or len(pair) != 2):
                raise ValueError(f"{name} must be None or a pair, got {pair!r}")
        self.n_cls, self.normalize, self.degrees, self.flip = n_cls, normalize, tuple(degrees), flip
        self.erase, self.zoom, self.gamma, self.noise = erase, zoom, gamma, bool(noise)

    @classmethod
    def from_ids(cls, n_cls, transform_2d, train=True):
        """The chain the reference builds from config.py's transform_2d (trainer.py:152-176): ids into its list, in
        ascending order as every configuration of the reference has them.  train=False keeps MRNormalize (1) and
        To_Tensor (10) only.  CropResize (2), RandomDistort2D (5) and Trunc_and_Normalize (11) raise ValueError by
        name; To_Tensor (10) must be present, the chain ends in the one-hot."""
        ids = [int(i) for i in transform_2d]
        for i in ids:
            if i not in TRANSFORM_2D_NAMES:
                raise ValueError(f"transform_2d id {i} is not in the reference's list (1..11)")
            if i in _REFUSED_2D:
                raise ValueError(f"transform_2d id {i} ({TRANSFORM_2D_NAMES[i]}) does not run on the device: "
                                 f"{_REFUSED_2D[i]}")
        if ids != sorted(set(ids)):
            raise ValueError(f"transform_2d must list each id once, in ascending order, got {ids}")
        if 10 not in ids:
            raise ValueError("transform_2d must hold 10 (To_Tensor): the chain returns the one-hot")
        if not train:
            ids = [i for i in ids if i in (1, 10)]
        return cls(n_cls, normalize="mr" if 1 in ids else None, degrees=REFERENCE_DEGREES if 6 in ids else (),
                   flip="hv" if 7 in ids else "", erase=(64, 64) if 3 in ids else None,
                   zoom=(0.8, 1.2) if 4 in ids else None, gamma=(0.8, 1.2) if 8 in ids else None, noise=9 in ids)

    def __call__(self, image, labels):
        """image: raw fp32 [B, C, H, W], labels: uint8 [B, H, W], both on the device.  Returns (image [B, C, H, W],
        onehot [B, n_cls, H, W]); the arguments are left untouched.  Per sample the draws follow the chain: erase and
        zoom (random), the degree (random), the flip (np.random), the gamma and the noise flag (random); after the
        batch, one np.random.randint for the noise seed when noise is on.  With erase or zoom on, the labels' bounding
        boxes come to the host in one copy before the draws (the only synchronisation of the call)."""
        if not torch.is_tensor(image) or image.device.type != "cuda":
            raise _lib.HdfError("TrainTransform2D needs device tensors (there is no CPU path)")
        if image.dim() != 4:
            raise ValueError(f"image must be [B, C, H, W], got {tuple(image.shape)}")
        image = image.clone(memory_format=torch.contiguous_format)     # the normalisation works in place
        labels = labels.contiguous()
        b, c, h, w = (int(s) for s in image.shape)
        if self.normalize == "mr":
            planes = image.view(b * c, 1, h, w)
            for k in range(0, b * c, 64):                              # the channel cap of hdf_normalize_mr
                mr_normalize_(planes[k:k + 64])
        moves = self.erase is not None or self.zoom is not None
        shades = self.gamma is not None or self.noise
        if not self.degrees and not self.flip and not moves and not shades:
            return image, onehot_from_labels(labels, self.n_cls)
        d = self.draw(b, h, w, label_bbox_2d(labels).cpu().numpy() if moves else None)
        if moves:
            image, labels = zoom_2d(image, labels, d["keeps"], d["canvases"])
        out_image, onehot = augment_2d(image, labels, self.n_cls, d["matrices"], d["flips"])
        if shades:
            intensity_2d_(out_image, d["gammas"], d["noise"], d["seed"], 0.0)
        return out_image, onehot

    def draw(self, batch, h, w, bbox=None):
        """The random parameters of one batch of `batch` h x w samples, drawn in the reference's order and nothing else:
        per sample erase and zoom (random; bbox [batch][5] from label_bbox_2d, needed when either is on), the degree
        (random), the flip (np.random), the gamma and the noise flag (random); then one np.random.randint for the noise
        seed when noise is on.  A transform that is off draws nothing and gives its neutral parameter.  Returns a dict:
        keeps, canvases, matrices, flips, gammas, noise (lists of `batch`) and seed."""
        if (self.erase is not None or self.zoom is not None) and bbox is None:
            raise ValueError("erase and zoom need the labels' bounding boxes")
        d = {k: [] for k in ("keeps", "canvases", "matrices", "flips", "gammas", "noise")}
        for k in range(batch):
            d["keeps"].append(erase2d_keep(bbox[k], h, w, self.erase) if self.erase is not None else (0, h, 0, w))
            d["canvases"].append(zoom2d_canvas(bbox[k], h, w, self.zoom) if self.zoom is not None else (w, h, 0, 0))
            d["matrices"].append(rotate_matrix(rotate_degree(self.degrees) if self.degrees else 0, w, h))
            d["flips"].append(flip2d_code(self.flip))
            d["gammas"].append(gamma2d(self.gamma) if self.gamma is not None else 1.0)
            d["noise"].append(int(noise2d_flag()) if self.noise else 0)
        d["seed"] = int(np.random.randint(0, 2 ** 63 - 1, dtype=np.int64)) if self.noise else 0
        return d
