"""The reference's 3-D training transform chain on the device (trainer.py:128-146 with config.py's
transform_3d = [1,2,4,5,6]): RandomCrop3D is a slice, PETandCTNormalize / MRNormalize the in-place kernels of
hdf_rt.inference, and RandomTranslationRotationZoom3D + RandomFlip3D + To_Tensor ONE gather kernel per sample
(hdf_augment_3d, csrc/augment.hip).  The random draws stay on the host and follow the reference's order, so seeding
np.random / random reproduces its parameters.  No CPU fallback.

The default 2-D chain (trainer.py:152-172 with config.py's transform_2d = [1,6,7,10]): MRNormalize per plane, then
RandomRotate2D + RandomFlip2D + To_Tensor ONE gather kernel per batch (hdf_augment_2d), bit for bit what PIL computes
on the host (pinned to PIL 12.2.0; include/hdf.h).  The matrix is built here, in Python, because PIL rounds the cosine
and the sine with Python's decimal round(., 15)."""
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


class TrainTransform3D:
    """transform_3d = [1,2,4,5,6] (normalize='petct') or [1,8,4,5,6] ('mr') of trainer.py:128-146 on device tensors:
    RandomCrop3D -> normalisation -> RandomTranslationRotationZoom3D(mode) -> RandomFlip3D(flip) -> To_Tensor.
    mode='' and flip='' give the validation chain (trainer.py:147-150: crop, normalise, one-hot).  The crop comes before
    the warp, so the warp's zero border is the border of the crop."""

    def __init__(self, n_cls, patch_size=None, normalize=None, mode="tr", flip="hv"):
        if normalize not in (None, "petct", "mr"):
            raise ValueError(f"normalize must be None, 'petct' or 'mr', got {normalize!r}")
        self.n_cls, self.patch_size, self.normalize, self.mode, self.flip = n_cls, patch_size, normalize, mode, flip

    def __call__(self, image, labels):
        """image: raw fp32 [C, Ds, Hs, Ws], labels: uint8 [Ds, Hs, Ws], both on the device.  Returns (image [C, D, H, W],
        onehot [n_cls, D, H, W]); the arguments are left untouched."""
        if not torch.is_tensor(image) or image.device.type != "cuda":
            raise _lib.HdfError("TrainTransform3D needs device tensors (there is no CPU path)")
        if self.patch_size is not None:
            p = tuple(int(v) for v in self.patch_size)
            o = crop_origin(labels.shape, p)
            image = image[:, o[0]:o[0] + p[0], o[1]:o[1] + p[1], o[2]:o[2] + p[2]]
            labels = labels[o[0]:o[0] + p[0], o[1]:o[1] + p[1], o[2]:o[2] + p[2]]
        image = image.clone(memory_format=torch.contiguous_format)     # the normalisation works in place
        labels = labels.contiguous()
        if self.normalize == "petct":
            pet_ct_normalize_(image)
        elif self.normalize == "mr":
            mr_normalize_(image)
        if not self.mode and not self.flip:
            return image, onehot_from_labels(labels[None], self.n_cls)[0]
        return augment_3d(image, labels, self.n_cls, trz_matrix(self.mode), *flip_flags(self.flip))


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


class TrainTransform2D:
    """transform_2d = [1,6,7,10] of trainer.py:152-172 on a device batch: MRNormalize (normalize='mr') ->
    RandomRotate2D(degrees) -> RandomFlip2D(flip) -> To_Tensor.  degrees=() and flip='' give the validation chain
    (trainer.py:173-176: normalise, one-hot).  MRNormalize works per plane, so a batch is simply more channels."""

    def __init__(self, n_cls, normalize="mr", degrees=REFERENCE_DEGREES, flip="hv"):
        if normalize not in (None, "mr"):
            raise ValueError(f"normalize must be None or 'mr', got {normalize!r}")
        self.n_cls, self.normalize, self.degrees, self.flip = n_cls, normalize, tuple(degrees), flip

    def __call__(self, image, labels):
        """image: raw fp32 [B, C, H, W], labels: uint8 [B, H, W], both on the device.  Returns (image [B, C, H, W],
        onehot [B, n_cls, H, W]); the arguments are left untouched.  Per sample the degree is drawn first (random),
        the flip second (np.random), as the reference's chain does."""
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
        if not self.degrees and not self.flip:
            return image, onehot_from_labels(labels, self.n_cls)
        mats, codes = [], []
        for _ in range(b):
            mats.append(rotate_matrix(rotate_degree(self.degrees) if self.degrees else 0, w, h))
            codes.append(flip2d_code(self.flip))
        return augment_2d(image, labels, self.n_cls, mats, codes)
