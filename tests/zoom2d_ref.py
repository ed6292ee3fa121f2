"""Restatement of the 2-D erase / zoom / gamma / noise transforms (data_utils/transformer_2d.py: RandomErase2D :11-77,
RandomZoom2D :177-275, RandomAdjust2D :279-305, RandomNoise2D :308-322) in plain numpy: the inputs of the tests of
hdf_label_bbox_2d, hdf_zoom_2d and hdf_intensity_2d (include/hdf.h) and their reference.  The zoom's contract is EXACT:
tests/test_zoom2d_ref_cpu.py holds this file bit for bit against PIL 12.2.0 (recorded in tests/golden/zoom2d_pil.npz,
and live where PIL is importable).

Semantics restated:
  erase: image pixels outside the keep-rectangle rows [r0, r1) x columns [c0, c1) read as 0.0f; labels are not touched
  canvas (sw, sh, ox, oy): sw wide, sh high; pixel (cy, cx) is the (erased) source pixel (cy - oy, cx - ox) when that
      lies inside the plane, else 0.  PIL's crop((x1, y1, x1+tw, y1+th)) is (tw, th, -x1, -y1); ImageOps.expand(border=
      (p0, p1, tw-W, th-H), fill=0) is (tw+p0, th+p1, p0, p1)
  image (ImagingResample, bilinear): horizontal pass, rounded to fp32, then vertical pass; a pass whose input and output
      sizes agree is skipped.  Per axis, in fp64 with every operation rounded: scale = n_in / n_out, fs = max(scale, 1),
      support = fs, centre = (xx + 0.5) scale, xmin = max((int)(centre - support + 0.5), 0), xmax = min((int)(centre +
      support + 0.5), n_in), w = 1 - |t| for |t| < 1 else 0 with t = (x + xmin - centre + 0.5) (1 / fs), k = w / sum(w);
      out = float32(sum(float64(pixel) k)), both sums left to right from 0.0
  labels (ImagingScaleAffine, nearest): a0 = n_in / n_out; the RUNNING sum xo = a0 0.5, then per output index
      src = (int)xo, xo += a0; the raw byte moves unchanged
  gamma: float32(pow(float64(x), float64(float32(gamma)))) for x > 0, else 0; gamma == 1 leaves the bits alone
  noise: clip(x + 0.1 z, low_clip, 1) with z = sqrt(-2 ln u1) cos(2 pi u2) from Philox-4x32-10 keyed by the seed on the
      counter (element index low, high, sample, 0): u1 = ((w0 << 20 | w1 >> 12) + 0.5) 2^-52, u2 = (w2 + 0.5) 2^-32"""
import numpy as np

from augment2d_ref import check_exact, image_of, labels_of  # noqa: F401  (shared inputs and checker)

SHAPES = ((24, 24), (37, 43), (43, 37), (96, 128))                              # (H, W)
FACTORS = (0.8, 0.83, 0.9, 0.999, 1.0, 1.01, 1.1, 1.2, 0.5, 2.0)
SCALES = (1.0, 1000.0)


# ------------------------------------------------------------------------------------------------------------ canvas
def crop_canvas(x1, y1, tw, th):
    """the canvas of PIL's crop((x1, y1, x1 + tw, y1 + th))"""
    return (int(tw), int(th), -int(x1), -int(y1))


def expand_canvas(p0, p1, tw, th):
    """the canvas of ImageOps.expand(border=(p0, p1, tw - W, th - H), fill=0)"""
    return (int(tw) + int(p0), int(th) + int(p1), int(p0), int(p1))


def erase(image, keep):
    """image [..., H, W] with everything outside rows [r0, r1) x columns [c0, c1) set to 0"""
    r0, r1, c0, c1 = keep
    out = np.zeros_like(image)
    out[..., r0:r1, c0:c1] = image[..., r0:r1, c0:c1]
    return out


def canvas_of(plane, canvas):
    """[sh, sw] of plane's dtype: plane [H, W] placed at (oy, ox), zero elsewhere"""
    sw, sh, ox, oy = canvas
    h, w = plane.shape
    out = np.zeros((sh, sw), dtype=plane.dtype)
    cy0, cy1, cx0, cx1 = max(oy, 0), min(oy + h, sh), max(ox, 0), min(ox + w, sw)
    if cy1 > cy0 and cx1 > cx0:
        out[cy0:cy1, cx0:cx1] = plane[cy0 - oy:cy1 - oy, cx0 - ox:cx1 - ox]
    return out


# ---------------------------------------------------------------------------------------------------- bilinear resize
def axis_coefficients(n_in, n_out, widen=True):
    """[(xmin, [k ...])] per output index, precompute_coeffs of PIL's Resample.c for the bilinear filter as Python floats
    (IEEE doubles, nothing fused).  widen=False: a planted defect, the support kept at 1 when shrinking"""
    scale = float(n_in) / n_out
    fs = max(scale, 1.0) if widen else 1.0
    support = 1.0 * fs
    ss = 1.0 / fs
    out = []
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in)
        ws, ww = [], 0.0
        for x in range(xmax - xmin):
            t = abs((x + xmin - center + 0.5) * ss)
            w = 1.0 - t if t < 1.0 else 0.0
            ws.append(w)
            ww += w
        out.append((xmin, [w / ww for w in ws] if ww != 0.0 else ws))
    return out


def resample_last_axis(a, n_out, widen=True):
    """one pass along the last axis of a [..., n_in], returned in fp64 (the caller rounds); None when it is skipped"""
    n_in = a.shape[-1]
    if n_in == n_out:
        return None
    a64 = a.astype(np.float64)
    out = np.empty(a.shape[:-1] + (n_out,), dtype=np.float64)
    for xx, (xmin, ks) in enumerate(axis_coefficients(n_in, n_out, widen)):
        ss = np.zeros(a.shape[:-1], dtype=np.float64)
        for j, k in enumerate(ks):
            ss = ss + a64[..., xmin + j] * np.float64(k)
        out[..., xx] = ss
    return out


def resize_bilinear(canvas, w, h, fp64_intermediate=False, widen=True):
    """fp32 [sh, sw] -> fp32 [h, w]; fp64_intermediate: a planted defect, the horizontal result not rounded to fp32"""
    canvas = np.asarray(canvas, dtype=np.float32)
    hor = resample_last_axis(canvas, w, widen)
    if hor is None:
        hor = canvas
    elif not fp64_intermediate:
        hor = hor.astype(np.float32)
    ver = resample_last_axis(hor.T, h, widen)
    return np.ascontiguousarray(hor if ver is None else ver.T).astype(np.float32)


# ----------------------------------------------------------------------------------------------------- nearest resize
def nearest_table(n_in, n_out, closed_form=False):
    """source index per output index: ImagingScaleAffine's running sum; closed_form: a planted defect,
    (int)((x + 0.5) a0)"""
    a0 = float(n_in) / n_out
    if closed_form:
        return np.array([int((x + 0.5) * a0) for x in range(n_out)], dtype=np.int64)
    tab, xo = [], a0 * 0.5
    for _ in range(n_out):
        tab.append(int(xo))
        xo += a0
    return np.array(tab, dtype=np.int64)


def resize_nearest(canvas, w, h, closed_form=False):
    """uint8 [sh, sw] -> uint8 [h, w]; an index past the canvas (it does not occur within the size limits) gives 0"""
    canvas = np.asarray(canvas, dtype=np.uint8)
    sh, sw = canvas.shape
    xi, yi = nearest_table(sw, w, closed_form), nearest_table(sh, h, closed_form)
    inside = (yi < sh)[:, None] & (xi < sw)[None, :]
    return np.where(inside, canvas[np.minimum(yi, sh - 1)[:, None], np.minimum(xi, sw - 1)[None, :]], 0).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------- one sample
def zoom_image(image, keep, canvas, erase_last=False, **defects):
    """image fp32 [C, H, W] -> fp32 [C, H, W]; erase_last: a planted defect, the erase applied after the resample"""
    h, w = image.shape[-2:]
    src = image if erase_last else erase(image, keep)
    out = np.stack([resize_bilinear(canvas_of(ch, canvas), w, h, **defects) for ch in src])
    return erase(out, keep) if erase_last else out


def zoom_labels(labels, canvas, closed_form=False):
    h, w = labels.shape
    return resize_nearest(canvas_of(labels, canvas), w, h, closed_form)


def zoom2d_batch_ref(image, labels, keeps, canvases):
    """a batch: image [B, C, H, W], labels [B, H, W], keeps [B][4], canvases [B][4] -> dict image, labels"""
    return {"image": np.stack([zoom_image(image[b], keeps[b], canvases[b]) for b in range(len(image))]),
            "labels": np.stack([zoom_labels(labels[b], canvases[b]) for b in range(len(labels))])}


def full_keep(h, w):
    return (0, h, 0, w)


# ------------------------------------------------------------------------------------------------------ PIL, for real
def pil_zoom(plane, factor, x1=0, y1=0, p0=0, p1=0):
    """what RandomZoom2D does to one plane (fp32 -> mode F + BILINEAR, uint8 -> mode L + NEAREST) at a given factor with
    given draws, through real crop / ImageOps.expand / resize calls; returns (result, canvas)"""
    from PIL import Image, ImageOps
    h, w = plane.shape
    tw, th = int(w * factor), int(h * factor)
    im = Image.fromarray(plane)
    if factor < 1.0:
        im, canvas = im.crop((x1, y1, x1 + tw, y1 + th)), crop_canvas(x1, y1, tw, th)
    else:
        im, canvas = ImageOps.expand(im, border=(p0, p1, tw - w, th - h), fill=0), expand_canvas(p0, p1, tw, th)
    assert im.size == canvas[:2], (im.size, canvas)
    im = im.resize((w, h), Image.BILINEAR if plane.dtype == np.float32 else Image.NEAREST)
    return np.array(im).astype(plane.dtype), canvas


def zoom_cases(shape, factor):
    """the draws tried per (shape, factor): (x1, y1, p0, p1); below 1 a crop inside the plane and two that leave it (a
    negative origin, and one past the far edge); from 1 on no shift and a shifted paste"""
    h, w = shape
    tw, th = int(w * factor), int(h * factor)
    if factor < 1.0:
        return ((0, 0, 0, 0), ((w - tw) // 2, h - th, 0, 0), (-3, -2, 0, 0), (w - tw + 4, 1, 0, 0))
    return ((0, 0, 0, 0), (0, 0, (tw - w) // 2, (th - h) // 3)) if tw > w or th > h else ((0, 0, 0, 0),)


# ------------------------------------------------------------------------------------------------------- label bbox
def bbox_ref(labels):
    """int32 [B][5]: (non-zero count, rmin, rmax, cmin, cmax) per sample; (0, H, -1, W, -1) for an empty one"""
    out = np.empty((len(labels), 5), dtype=np.int32)
    for b, lab in enumerate(labels):
        r, c = np.nonzero(lab)
        out[b] = (len(r), r.min(), r.max(), c.min(), c.max()) if len(r) else (0, lab.shape[0], -1, lab.shape[1], -1)
    return out


# -------------------------------------------------------------------------------------------------- gamma and noise
def gamma_ref(x, gamma):
    """fp32 array -> fp32: pow in fp64 on the fp32-rounded gamma, one rounding; x <= 0 gives 0; gamma == 1: untouched"""
    x = np.asarray(x, dtype=np.float32)
    g = np.float64(np.float32(gamma))
    if g == 1.0:
        return x.copy()
    out = np.zeros_like(x)
    pos = x > 0
    out[pos] = np.power(x[pos].astype(np.float64), g).astype(np.float32)
    return out


_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32(counter, key):
    """Philox-4x32-10: counter four uint64 arrays holding 32-bit words, key two Python ints; returns four uint64 arrays of
    32-bit words"""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & _MASK for c in counter)
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c0, np.uint64(_M1) * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & _MASK,
                          (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & _MASK)
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def normal_ref(seed, sample, n):
    """z fp64 [n] of one sample: element index i in [0, n)"""
    i = np.arange(n, dtype=np.uint64)
    w0, w1, w2, _ = philox4x32((i & _MASK, i >> np.uint64(32), np.full(n, sample, dtype=np.uint64), np.zeros(n, np.uint64)),
                               (seed & 0xFFFFFFFF, seed >> 32))
    u1 = (((w0 << np.uint64(20)) | (w1 >> np.uint64(12))).astype(np.float64) + 0.5) * 2.0 ** -52
    u2 = (w2.astype(np.float64) + 0.5) * 2.0 ** -32
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def intensity_ref(image, gammas, noise, seed, low_clip):
    """image fp32 [B, C, H, W] -> fp32: gamma per sample, then noise where noise[b]"""
    out = np.empty_like(image)
    for b in range(len(image)):
        x = gamma_ref(image[b], gammas[b])
        if noise[b]:
            z = normal_ref(seed, b, x.size).reshape(x.shape)
            x = np.clip(x.astype(np.float64) + 0.1 * z, np.float64(np.float32(low_clip)), 1.0).astype(np.float32)
        out[b] = x
    return out
