"""fp64 restatement of the resize of the reference's CropResize (data_utils/data_loader.py:103-119) in numpy, and the
literal scipy sequence it restates.

skimage.transform.resize(x, dim, order=1) on an fp32 array is, since scikit-image 0.19, scipy: per axis f = n_in / n_out,
sigma = max(0, (f - 1) / 2) (anti-aliasing; the labels' anti_aliasing=None resolves to "some axis shrinks", and sigma is 0 on
every axis that does not), ndimage.gaussian_filter(x, sigma, mode=M, cval=0) -- truncate 4: radius int(4 sigma + 0.5),
weights exp(-0.5 k^2 / sigma^2) normalised; an axis with sigma <= 1e-15 is skipped -- then ndimage.zoom(., n_out / n_in,
order=1, mode=M, cval=0, grid_mode=True): output o reads c = (o + 0.5) f - 0.5, linear between floor(c) and floor(c) + 1.
M = 'mirror' for the image (index p -> |p| mod (2n - 2), folded back when >= n; 0 when n = 1) and 'grid-constant' for the
per-class label masks (a sample outside [0, n) is 0, in the filter and in the interpolation).

Restated here: one axis is the dense matrix Z @ G (interpolation rows times filter rows) in fp64; the three matrices are
applied one after the other in fp64 and nothing is rounded in between.  scipy rounds to fp32 after every filtered axis and
after the zoom, so it differs from this by at most (g + 1) 2^-24 vmax, g the number of filtered axes.
tests/test_resize_ref_cpu.py holds this file against live scipy and shows that the checks reject five planted defects."""
import numpy as np

from augment_ref import labels_from_sums      # the loop of data_loader.py:114-118 is that of transformer_3d.py:113-116

# in -> out, the cases of the resize tests (what each exercises: tests/test_resize_ref_cpu.py)
SHAPES = [((9, 37, 43), (6, 24, 48)), ((5, 20, 22), (7, 31, 29)), ((8, 37, 43), (1, 24, 48)), ((1, 37, 43), (1, 24, 48)),
          ((16, 3, 8), (2, 3, 1)), ((7, 40, 48), (7, 20, 24)), ((104, 101, 103), (53, 80, 111))]
BIG = SHAPES[-1]


def sigma_of(n_in, n_out):
    return max(0.0, (n_in / n_out - 1.0) / 2.0)


def boundary(p, n, mode, reflect=False):
    """source index of p on an axis of n samples, or None when it reads as 0.  reflect: the planted defect, scipy's
    'reflect' (d c b a | a b c d) in place of 'mirror' (d c b | a b c d)"""
    if mode == "constant":
        return p if 0 <= p < n else None
    if reflect:
        q = p % (2 * n)
        return 2 * n - 1 - q if q >= n else q
    if n == 1:
        return 0
    q = abs(p) % (2 * n - 2)
    return 2 * n - 2 - q if q >= n else q


def axis_operator(n_in, n_out, mode, reflect=False, radius_floor=False, no_half=False):
    """the dense [n_out, n_in] fp64 matrix of one axis, and whether the axis is filtered.  The keyword arguments plant a
    defect each: 'reflect' for 'mirror', r = int(4 sigma), c = (o + 0.5) f without the - 0.5."""
    f = n_in / n_out
    sigma = sigma_of(n_in, n_out)
    filtered = sigma > 1e-15
    g = np.zeros((n_in, n_in))
    if filtered:
        r = int(4.0 * sigma) if radius_floor else int(4.0 * sigma + 0.5)
        k = np.arange(-r, r + 1)
        w = np.exp(-0.5 / (sigma * sigma) * k ** 2)
        w = w / w.sum()
        for j in range(n_in):
            for kk, wk in zip(k, w):
                q = boundary(j + int(kk), n_in, mode, reflect)
                if q is not None:
                    g[j, q] += wk
    else:
        g[np.arange(n_in), np.arange(n_in)] = 1.0
    z = np.zeros((n_out, n_in))
    for o in range(n_out):
        c = (o + 0.5) * f - (0.0 if no_half else 0.5)
        i0 = int(np.floor(c))
        t = c - i0
        for i, wt in ((i0, 1.0 - t), (i0 + 1, t)):
            q = boundary(i, n_in, mode, reflect)
            if q is not None and wt != 0.0:
                z[o, q] += wt
    return z @ g, filtered


def resize_plane(x, out_shape, mode, **defect):
    """one [D, H, W] plane through the three operators in fp64; returns (fp64 plane, g)"""
    y = np.asarray(x, dtype=np.float64)
    g = 0
    for a in range(3):
        m, filtered = axis_operator(y.shape[a], out_shape[a], mode, **defect)
        g += int(filtered)
        y = np.moveaxis(np.tensordot(m, y, axes=([1], [a])), 0, a)
    return y, g


def resize_ref(image, labels, n_cls, out_shape, **defect):
    """dict: image fp64 [C, *out_shape] (None without an image), sums fp64 [n_cls - 1, *out_shape] and labels uint8 (None
    without labels), g the number of filtered axes"""
    out = {"image": None, "sums": None, "labels": None, "g": 0}
    if image is not None:
        planes = [resize_plane(ch, out_shape, "mirror", **defect) for ch in image]
        out["image"], out["g"] = np.stack([p[0] for p in planes]), planes[0][1]
    if labels is not None:
        planes = [resize_plane(labels == z, out_shape, "constant", **defect) for z in range(1, n_cls)]
        out["sums"], out["g"] = np.stack([p[0] for p in planes]), planes[0][1]
        out["labels"] = labels_from_sums(out["sums"])
    return out


# -------------------------------------------------------------------------------------------------------------- scipy
def scipy_plane(x, out_shape, mode, anti_aliasing=True):
    """the literal sequence of skimage.transform.resize(order=1) on one fp32 plane: gaussian_filter, then
    zoom(grid_mode=True), both in fp32 arrays"""
    from scipy import ndimage as ndi
    x = np.asarray(x, dtype=np.float32)
    m = {"mirror": "mirror", "constant": "grid-constant"}[mode]
    if anti_aliasing:
        sigma = [sigma_of(i, o) for i, o in zip(x.shape, out_shape)]
        x = ndi.gaussian_filter(x, sigma, mode=m, cval=0)
    out = ndi.zoom(x, [o / i for i, o in zip(x.shape, out_shape)], order=1, mode=m, cval=0, grid_mode=True)
    assert out.shape == tuple(out_shape) and out.dtype == np.float32, (out.shape, out.dtype)
    return out


def scipy_pipeline(image, labels, n_cls, out_shape):
    """CropResize's resize as the reference runs it, in fp32: (image fp32 [C, *out_shape], sums fp32 [n_cls - 1,
    *out_shape], labels uint8); None for what was not given"""
    img = None if image is None else np.stack([scipy_plane(ch, out_shape, "mirror") for ch in image])
    if labels is None:
        return img, None, None
    shrinks = any(o < i for i, o in zip(labels.shape, out_shape))
    sums = np.stack([scipy_plane((labels == z).astype(np.float32), out_shape, "constant", shrinks)
                     for z in range(1, n_cls)])
    return img, sums, labels_from_sums(sums)


# ----------------------------------------------------------------------------------------------------------- checkers
def check_against_scipy(ref64, got32, g, vmax, what="image"):
    """per element |scipy - restatement| <= (g + 1) 2^-24 vmax: scipy rounds to fp32 once per filtered axis and once
    after the zoom, each time by at most half an ulp of a value bounded by vmax (every operator row is a convex
    combination, or a sub-convex one under 'grid-constant').  Returns the worst error in units of 2^-24 vmax."""
    ref64, got = np.asarray(ref64, dtype=np.float64), np.asarray(got32, dtype=np.float64)
    assert ref64.shape == got.shape, (ref64.shape, got.shape)
    unit = 2.0 ** -24 * float(vmax)
    err = np.abs(got - ref64) / unit
    bad = ~(err <= g + 1)
    if bad.any():
        k = np.unravel_index(int(np.nanargmax(np.where(np.isnan(err), np.inf, err))), err.shape)
        raise AssertionError("%s: %d of %d elements outside the bound; worst at %s: scipy %.9g, restatement %.17g, %.3f "
                             "units against %d" % (what, int(bad.sum()), err.size, k, got[k], ref64[k], err[k], g + 1))
    return float(err.max())


def band(sums64):
    """voxels where some class sum lies within 1e-7 of 0.5: scipy's decision there is its own rounding noise"""
    return (np.abs(np.asarray(sums64) - 0.5) <= 1e-7).any(0)


def check_maps_outside_band(want, got, sums64, what="labels"):
    """the class maps agree at every voxel outside the band; returns the band's share"""
    want, got = np.asarray(want), np.asarray(got)
    assert want.shape == got.shape and got.dtype == np.uint8, (want.shape, got.shape, got.dtype)
    wrong = (want != got) & ~band(sums64)
    assert not wrong.any(), "%s: %d voxels differ outside the band, first at %s" % (
        what, int(wrong.sum()), tuple(np.argwhere(wrong)[0]))
    return float(band(sums64).mean())
