"""Restatement of the reference's default 2-D training chain after the normalisation (data_utils/transformer_2d.py:
RandomRotate2D :134-173, RandomFlip2D :80-132, To_Tensor of data_utils/data_loader.py:126-159) in vectorised numpy, the
inputs of the 2-D augmentation tests and their checker.  The contract is EXACT: tests/test_augment2d_ref_cpu.py holds
this file bit for bit against PIL (recorded in tests/golden/augment2d_pil.npz, and live where PIL is importable).

Semantics restated (m = (a, b, c, d, e, f), PIL's Image.transform(AFFINE) convention, output pixel -> input coordinate):
  matrix: PIL's Image.rotate: ang = -radians(angle % 360), centre (W/2, H/2) (not (W-1)/2), cosine and sine rounded with
      Python's round(., 15)
  image (affine_transform + bilinear_filter32F): xin = a (x+.5) + b (y+.5) + c, yin likewise, left to right in fp64;
      0 outside [0, W) x [0, H); else minus 0.5, floor, rows and columns clamped; v1 = p0 + float32(p1 - p0) * dx -- the
      neighbour difference is an fp32 subtraction --; v2 the same on row y0 + 1 when that row exists, else v1;
      out = float32(v1 + (v2 - v1) dy)
  labels (affine_fixed): 16.16 fixed point, FIX(v) = floor(v 65536 + 0.5); the byte at ((a2 + y a1 + x a0) >> 16,
      (a5 + y a4 + x a3) >> 16) when inside, else 0; the raw byte moves unchanged
  flip AFTER the rotation: 1 mirrors W, 2 mirrors H; one-hot channel z >= 1 is (label == z), channel 0 "no other class"."""
import math

import numpy as np

SHAPES = ((24, 24), (17, 29), (40, 33), (37, 43), (1, 9), (9, 1), (2, 2))      # (H, W)
ANGLES = (-15, -10, -5, 0, 5, 10, 15, 90, 180, 270, 37.3, 181)
REFERENCE_DEGREES = (-15, -10, -5, 0, 5, 10, 15)                                # transformer_2d.py:144
SCALES = (1.0, 100.0, 1e-3)
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)


# ------------------------------------------------------------------------------------------------------------ inputs
def image_of(shape, channels, seed, scale=1.0):
    """fp32 [C, H, W], both signs in every channel, times `scale`"""
    rng = np.random.RandomState(seed)
    return (rng.standard_normal((channels,) + tuple(shape)) * scale).astype(np.float32)


def labels_of(shape, seed, blocky=None):
    """uint8 [H, W] holding 0..3, 200 and 255 (the last two match no class of n_cls <= 8).  blocky (the default where
    both sides exceed 2): classes per 3x4 block with a few strays of 200 and 255; otherwise the six values in equal
    shares, shuffled per pixel, so that a map of six pixels or more holds them all"""
    rng = np.random.RandomState(seed + 1000)
    size = int(shape[0]) * int(shape[1])
    if blocky is None:
        blocky = min(shape) > 2
    if not blocky:
        return rng.permutation(np.resize(np.array([0, 1, 2, 3, 200, 255], dtype=np.uint8), size)).reshape(shape)
    small = rng.randint(0, 4, size=(-(-shape[0] // 3), -(-shape[1] // 4)))
    lab = np.ascontiguousarray(np.kron(small, np.ones((3, 4), dtype=np.int64))[:shape[0], :shape[1]]).astype(np.uint8)
    flat = lab.reshape(-1)
    pick = rng.choice(size, size=max(2, size // 40), replace=False)
    flat[pick[::2]] = 200
    flat[pick[1::2]] = 255
    return lab


# ------------------------------------------------------------------------------------------------------- restatement
def matrix_of(angle, width, height, centre=None):
    """the six doubles PIL's Image.rotate hands to Image.transform(AFFINE); centre: a planted defect only"""
    ang = -math.radians(angle % 360)
    cx, cy = (width / 2.0, height / 2.0) if centre is None else centre
    a, b = round(math.cos(ang), 15), round(math.sin(ang), 15)
    d, e = round(-math.sin(ang), 15), round(math.cos(ang), 15)
    c = (a * (-cx) + b * (-cy) + 0.0) + cx
    f = (d * (-cx) + e * (-cy) + 0.0) + cy
    return (a, b, c, d, e, f)


def source_coords(shape, m):
    """(xin, yin) fp64 [H, W] of every output pixel centre, the products summed left to right"""
    a, b, c, d, e, f = (np.float64(v) for v in m)
    x = np.arange(shape[1], dtype=np.float64)[None, :] + 0.5
    y = np.arange(shape[0], dtype=np.float64)[:, None] + 0.5
    return a * x + b * y + c, d * x + e * y + f


def rotate_image(ch, m, diff=np.float32):
    """one fp32 plane [H, W] through affine_transform + bilinear_filter32F; diff: the type of the neighbour difference
    (fp32 is PIL's; fp64 is a planted defect)"""
    ch = np.asarray(ch, dtype=np.float32)
    h, w = ch.shape
    xin, yin = source_coords(ch.shape, m)
    inside = ~((xin < 0) | (xin >= w) | (yin < 0) | (yin >= h))
    xin, yin = xin - 0.5, yin - 0.5
    x0, y0 = np.floor(xin), np.floor(yin)
    dx, dy = xin - x0, yin - y0
    x0 = np.where(inside, x0, 0).astype(np.int64)
    y0 = np.where(inside, y0, 0).astype(np.int64)
    xa, xb = np.clip(x0, 0, w - 1), np.clip(x0 + 1, 0, w - 1)

    def row(r):
        p0, p1 = ch[r, xa], ch[r, xb]
        return p0.astype(np.float64) + (p1.astype(diff) - p0.astype(diff)).astype(np.float64) * dx

    v1 = row(np.clip(y0, 0, h - 1))
    below = (y0 + 1 >= 0) & (y0 + 1 < h)
    v2 = np.where(below, row(np.clip(y0 + 1, 0, h - 1)), v1)
    return np.where(inside, v1 + (v2 - v1) * dy, 0.0).astype(np.float32)


def fix(v):
    return int(math.floor(v * 65536.0 + 0.5))


def fixed_coefficients(m):
    """(a0, a1, a2, a3, a4, a5) of affine_fixed as Python integers"""
    a, b, c, d, e, f = (float(v) for v in m)
    return fix(a), fix(b), fix(c + a * 0.5 + b * 0.5), fix(d), fix(e), fix(f + d * 0.5 + e * 0.5)


def passes_check_fixed(m, width, height):
    a, b, c, d, e, f = (float(v) for v in m)
    return all(abs(x * a + y * b + c) < 32768.0 and abs(x * d + y * e + f) < 32768.0
               for x, y in ((0, 0), (width, 0), (0, height), (width, height)))


def rotate_labels(lab, m, floor_of_fp64=False):
    """one uint8 map [H, W] through affine_fixed; floor_of_fp64: a planted defect, the nearest pixel taken at the floor of
    the fp64 coordinate instead of the 16.16 value"""
    lab = np.asarray(lab, dtype=np.uint8)
    h, w = lab.shape
    if floor_of_fp64:
        xin, yin = source_coords(lab.shape, m)
        xi, yi = np.floor(xin).astype(np.int64), np.floor(yin).astype(np.int64)
    else:
        a0, a1, a2, a3, a4, a5 = fixed_coefficients(m)
        x = np.arange(w, dtype=np.int64)[None, :]
        y = np.arange(h, dtype=np.int64)[:, None]
        xi, yi = (a2 + y * a1 + x * a0) >> 16, (a5 + y * a4 + x * a3) >> 16
    inside = (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h)
    return np.where(inside, lab[np.clip(yi, 0, h - 1), np.clip(xi, 0, w - 1)], 0).astype(np.uint8)


def flip(a, code):
    """1 mirrors W, 2 mirrors H, 0 nothing"""
    if code == 1:
        a = a[..., ::-1]
    elif code == 2:
        a = a[..., ::-1, :]
    return np.ascontiguousarray(a)


def onehot_of(labels, n_cls):
    """To_Tensor: channel z >= 1 is (label == z), channel 0 "no other class" (a value >= n_cls is background)"""
    oh = np.zeros((n_cls,) + labels.shape, dtype=np.float32)
    for z in range(1, n_cls):
        oh[z] = labels == z
    oh[0] = oh[1:].max(0) == 0
    return oh


def augment2d_ref(image, labels, n_cls, m, flip_code=0):
    """one sample: image fp32 [C, H, W], labels uint8 [H, W] -> dict image fp32, labels uint8, onehot fp32"""
    img = flip(np.stack([rotate_image(ch, m) for ch in image]), flip_code)
    lab = flip(rotate_labels(labels, m), flip_code)
    return {"image": img, "labels": lab, "onehot": onehot_of(lab, n_cls)}


def augment2d_batch_ref(image, labels, n_cls, matrices, flips):
    """a batch: image [B, C, H, W], labels [B, H, W], matrices [B][6], flips [B]"""
    per = [augment2d_ref(image[b], labels[b], n_cls, matrices[b], int(flips[b])) for b in range(len(image))]
    return {k: np.stack([p[k] for p in per]) for k in ("image", "labels", "onehot")}


# ----------------------------------------------------------------------------------------------------------- checker
def check_exact(got, want, what="output"):
    """bit equality: fp32 compared as uint32 (so -0.0 is not +0.0 and a NaN equals only itself), uint8 as bytes"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    same = got.view(np.uint32) == want.view(np.uint32) if got.dtype == np.float32 else got == want
    if not same.all():
        k = tuple(np.argwhere(~same)[0])
        raise AssertionError("%s: %d of %d elements differ, first at %s: got %r, want %r"
                             % (what, int((~same).sum()), same.size, k, got[k], want[k]))
