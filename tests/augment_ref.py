"""fp64 restatement of the reference's 3-D augmentation (data_utils/transformer_3d.py:45-169, To_Tensor of
data_utils/data_loader.py:126-159) in numpy, the inputs of the augmentation tests and their checkers.

Semantics restated:
  source coordinate of output voxel p:  c = A (p - s) + t + s,  s = size / 2  (not (size - 1) / 2)
  interpolation: skimage.transform.warp on a 3-D array = scipy.ndimage.map_coordinates(order=1, mode='grid-constant',
      cval=0): trilinear on the volume zero-padded to infinity -- eight corners, a corner outside contributes 0 -- in fp64
  labels: for z = 1 .. n_cls-1 ascending, new[warp(label == z) >= 0.5] = z: the last class reaching 0.5 wins, >= is
      inclusive, values >= n_cls match nothing
  flip AFTER the warp; one-hot channel 0 = "no other class".
tests/test_augment_ref_cpu.py holds this file against scipy and shows that the checkers reject six planted defects."""
import numpy as np

SHAPE = (5, 37, 43)                 # odd, W no multiple of any vector width
BIG_SHAPE = (104, 101, 103)         # the staging tests' volume: past every grid cap


def _rx(a):
    return np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]], dtype=np.float64)


def _ry(a):
    return np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], dtype=np.float64)


def _rz(a):
    return np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]], dtype=np.float64)


def _mat(rot, zoom, t):
    return np.concatenate([rot @ np.diag(np.asarray(zoom, dtype=np.float64)), np.asarray(t, dtype=np.float64)[:, None]], 1)


IDENTITY = _mat(np.eye(3), (1, 1, 1), (0, 0, 0))
# fixed draws inside the reference's ranges: mode 'tr', mode 'trz', and a general 3-axis rotation with zoom whose source
# coordinates leave the volume for a good part of the voxels
TR = _mat(_rx(np.deg2rad(3.7)), (1, 1, 1), (0, -4.3, 2.9))
TRZ = _mat(_rx(np.deg2rad(-4.6)), (1, 1.08, 0.93), (0, 3.1, -4.8))
ROT3 = _mat(_rz(np.deg2rad(9.0)) @ _ry(np.deg2rad(-14.0)) @ _rx(np.deg2rad(21.0)), (1.15, 0.9, 1.2), (0.7, -2.4, 3.3))
MATRICES = {"tr": TR, "trz": TRZ, "rot3": ROT3}


def translation(t):
    return _mat(np.eye(3), (1, 1, 1), t)


# ------------------------------------------------------------------------------------------------------------ inputs
def image_of(shape, channels, seed):
    """fp32 [C, D, H, W], both signs in every channel, the last channel scaled by 1e4"""
    rng = np.random.RandomState(seed)
    img = rng.standard_normal((channels,) + tuple(shape))
    img[-1] *= 1e4
    return img.astype(np.float32)


def labels_of(shape, n_cls, seed, blocky=False, strays=True):
    """uint8 [D, H, W]: uniform-random classes per voxel, or per 3x4x4 block; strays: a few voxels of 200 and 255, which
    no class of n_cls <= 8 matches"""
    rng = np.random.RandomState(seed + 1000)
    if blocky:
        small = rng.randint(0, n_cls, size=tuple(-(-s // b) for s, b in zip(shape, (3, 4, 4))))
        lab = np.kron(small, np.ones((3, 4, 4), dtype=np.int64))[:shape[0], :shape[1], :shape[2]]
    else:
        lab = rng.randint(0, n_cls, size=tuple(shape))
    lab = lab.astype(np.uint8)
    if strays:
        flat = lab.reshape(-1)
        pick = rng.choice(flat.size, size=max(2, flat.size // 50), replace=False)
        flat[pick[::2]] = 200
        flat[pick[1::2]] = 255
    return lab


# ------------------------------------------------------------------------------------------------------- restatement
def source_coords(shape, affine, centre=None):
    """c [3, D, H, W] fp64 = A (p - s) + t + s, the products summed left to right as numpy's dot does for one row"""
    m = np.asarray(affine, dtype=np.float64)
    s = [n / 2 for n in shape] if centre is None else list(centre)
    p = np.mgrid[:shape[0], :shape[1], :shape[2]].astype(np.float64)
    q = [p[k] - s[k] for k in range(3)]
    return np.stack([m[k, 0] * q[0] + m[k, 1] * q[1] + m[k, 2] * q[2] + m[k, 3] + s[k] for k in range(3)])


def corners(c, shape):
    """the eight corners of every source coordinate: flat offsets [8, D, H, W] (clipped into the volume) and fp64 weights
    [8, D, H, W], 0 for a corner outside the volume (the zero padding of `grid-constant`)"""
    fl = np.floor(c)
    fr = c - fl
    i0 = np.clip(fl, -2, np.asarray(shape, dtype=np.float64)[:, None, None, None]).astype(np.int64)
    offs, wts = [], []
    for k in range(8):
        bit = (k >> 2, (k >> 1) & 1, k & 1)
        idx = [i0[a] + bit[a] for a in range(3)]
        inside = np.ones(c.shape[1:], dtype=bool)
        for a in range(3):
            inside &= (idx[a] >= 0) & (idx[a] < shape[a])
        w = (fr[0] if bit[0] else 1 - fr[0]) * (fr[1] if bit[1] else 1 - fr[1]) * (fr[2] if bit[2] else 1 - fr[2])
        idx = [np.clip(idx[a], 0, shape[a] - 1) for a in range(3)]
        offs.append((idx[0] * shape[1] + idx[1]) * shape[2] + idx[2])
        wts.append(np.where(inside, w, 0.0))
    return np.stack(offs), np.stack(wts)


def interpolate(vol, offs, wts, dtype=np.float64):
    """sum over the eight corners of weight x value (accumulated in `dtype`: fp64 is the reference)"""
    flat = np.asarray(vol).reshape(-1).astype(dtype)
    acc = np.zeros(offs.shape[1:], dtype=dtype)
    for k in range(8):
        acc = acc + wts[k].astype(dtype) * flat[offs[k]]
    return acc


def labels_from_sums(sums, inclusive=True, last_wins=True):
    """sums [n_cls - 1, D, H, W] of classes 1 .. n_cls-1 -> uint8 class map"""
    out = np.zeros(sums.shape[1:], dtype=np.uint8)
    for k in range(sums.shape[0]):
        hit = sums[k] >= 0.5 if inclusive else sums[k] > 0.5
        if not last_wins:
            hit &= out == 0
        out[hit] = k + 1
    return out


def flip(a, flip_h, flip_w):
    if flip_h:
        a = a[..., ::-1, :]
    if flip_w:
        a = a[..., ::-1]
    return np.ascontiguousarray(a)


def onehot_of(labels, n_cls):
    """To_Tensor: channel z >= 1 is (label == z), channel 0 "no other class" """
    oh = np.zeros((n_cls,) + labels.shape, dtype=np.float32)
    for z in range(1, n_cls):
        oh[z] = labels == z
    oh[0] = oh[1:].max(0) == 0
    return oh


def class_sums(labels, n_cls, offs, wts):
    return np.stack([interpolate((labels == z).astype(np.float64), offs, wts) for z in range(1, n_cls)])


def augment_ref(image, labels, n_cls, affine, flip_h=False, flip_w=False):
    """dict: image fp64 [C, D, H, W], sums fp64 [n_cls-1, D, H, W], labels uint8, onehot fp32 (all after the flip) and
    `outside`, the share of voxels with at least one corner outside the volume"""
    shape = labels.shape
    offs, wts = corners(source_coords(shape, affine), shape)
    img = np.stack([interpolate(ch, offs, wts) for ch in image])
    sums = class_sums(labels, n_cls, offs, wts)
    lab = labels_from_sums(sums)
    lab = flip(lab, flip_h, flip_w)
    return {"image": flip(img, flip_h, flip_w), "sums": flip(sums, flip_h, flip_w), "labels": lab,
            "onehot": onehot_of(lab, n_cls), "outside": float((wts == 0).any(0).mean())}


# ----------------------------------------------------------------------------------------------------------- checkers
def check_image(got, ref64, vmax, what="image"):
    """per element |got - ref| <= 2^-23 |ref| + 1e-11 vmax.  First term: one fp32 rounding, times 2 for the reference's
    own last bit.  Second: coordinate rounding -- fp64 eps x about 5 operations x extent <= 200 is about 2e-13 per
    coordinate, x 3 axes x 8 corners x the largest corner magnitude vmax.  Returns the worst error / bound."""
    got, ref64 = np.asarray(got, dtype=np.float64), np.asarray(ref64, dtype=np.float64)
    assert got.shape == ref64.shape, (got.shape, ref64.shape)
    bound = 2.0 ** -23 * np.abs(ref64) + 1e-11 * float(vmax)
    ratio = np.abs(got - ref64) / bound
    bad = ~(ratio <= 1.0)                     # (a NaN compares false: a NaN output fails)
    if bad.any():
        k = np.unravel_index(int(np.nanargmax(np.where(np.isnan(ratio), np.inf, ratio))), ratio.shape)
        raise AssertionError("%s: %d of %d elements outside the bound; worst at %s: got %.9g, reference %.17g, %.3f x "
                             "the bound" % (what, int(bad.sum()), ratio.size, k, got[k], ref64[k], ratio[k]))
    return float(ratio.max())


def check_labels(got, sums64, what="labels"):
    """exact equality with the class map of sums64 everywhere except voxels where some class sum lies within 1e-7 of 0.5
    (the reference's own fp32 rounding of the sum); that share must be <= 1e-4 -- a condition on the inputs.  Returns the
    excluded share."""
    got = np.asarray(got)
    want = labels_from_sums(sums64)
    assert got.shape == want.shape, (got.shape, want.shape)
    excluded = (np.abs(sums64 - 0.5) <= 1e-7).any(0)
    share = float(excluded.mean())
    assert share <= 1e-4, "%s: %.2e of the voxels have a class sum within 1e-7 of 0.5" % (what, share)
    wrong = (got != want) & ~excluded
    assert not wrong.any(), "%s: %d voxels differ, first at %s" % (what, int(wrong.sum()), tuple(np.argwhere(wrong)[0]))
    return share


def check_exact(got, want, what="output"):
    """bit equality (the exact cases: identity, flips, integer and half-voxel translations)"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    same = got.view(np.uint8) == want.view(np.uint8) if got.dtype != np.uint8 else got == want
    assert same.all(), "%s: %d bytes differ" % (what, int((~same).sum()))
