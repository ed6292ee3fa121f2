"""CPU restatement of sliding-window inference with a Gaussian importance map and mirror test-time augmentation
(csrc/sw_infer.hip, hdf_rt.inference.sliding_window_predict): the importance map from its per-axis tables, the gather of a
window's mirrored copies, the accumulation in the kernel's order in fp64 or fp32, the whole loop, and the comparison that
the GPU tests hold the kernels to (tests/test_sw_ref_cpu.py shows that it rejects six planted defects).  torch / numpy only;
no GPU and no scipy in here -- tests/test_sw_ref_cpu.py pins the map to scipy.ndimage.gaussian_filter bit for bit."""
import numpy as np
import torch

from hip_util import check_fp32_sum

# the cases on which the map is pinned: zeros (replaced by the floor) occur at 1/16 and 1/32, (2, 2, 2) at 1/16 is denormal
EXTENTS = [(8, 8, 8), (7, 9, 5), (16, 12, 20), (1, 8, 8), (3, 2, 4), (32, 24, 17), (13, 13, 13), (2, 2, 2), (1, 1, 1),
           (48, 40, 33)]
SIGMA_SCALES = [1 / 8, 1 / 4, 1 / 16, 1 / 32]


def axis_table(n, sigma_scale, centre=None):
    """what a normalised Gaussian kernel of sigma = n * sigma_scale, cut at int(4 sigma + 0.5), leaves of a unit impulse
    at `centre` (n // 2) on an axis of length n whose outside is 0; fp64"""
    centre = n // 2 if centre is None else centre
    sigma = n * sigma_scale
    r = int(4.0 * sigma + 0.5)
    j = np.arange(-r, r + 1)
    k = np.exp(-0.5 / (sigma * sigma) * j ** 2)
    k /= k.sum()
    t = np.zeros(n)
    for i in range(n):
        if abs(i - centre) <= r:
            t[i] = k[i - centre + r]
    return t


def tables_of(extent, sigma_scale):
    return tuple(axis_table(int(n), sigma_scale) for n in extent)


def raw_weights(tables):
    """fp32 [ed, eh, ew]: ((tz * ty) * tx) / peak in fp64, in this order, rounded once; zeros still in place"""
    tz, ty, tx = tables
    peak = (tz[len(tz) // 2] * ty[len(ty) // 2]) * tx[len(tx) // 2]
    return (((tz[:, None, None] * ty[None, :, None]) * tx[None, None, :]) / peak).astype(np.float32)


def floor_of(raw):
    return raw[raw != 0].min()


def map_of(tables):
    """the importance map of a window from its three tables: zeros replaced by the smallest non-zero weight"""
    w = raw_weights(tables)
    w[w == 0] = floor_of(w)
    return w


def importance_map(extent, sigma_scale):
    return map_of(tables_of(extent, sigma_scale))


def variants(mask):
    """mirror codes (bit 0 = z, 1 = y, 2 = x) of the subsets of mask, ascending"""
    return [m for m in range(8) if m & ~mask == 0]


def mirror(t, m):
    """flip the last three axes [.., z, y, x] of t that the code m names"""
    dims = [d for b, d in ((1, -3), (2, -2), (4, -1)) if m & b]
    return torch.flip(t, dims) if dims else t


def gather_ref(image, origin, ext, patch, mask):
    """[K, C, Pd, Ph, Pw]: per variant the window's content mirrored within its clipped extent, then zero-padded up to the
    patch at the high end of every axis"""
    (z, y, x), (d, h, w) = origin, ext
    content = image[:, z:z + d, y:y + h, x:x + w]
    out = torch.zeros((len(variants(mask)), image.shape[0]) + tuple(patch), dtype=image.dtype)
    for k, m in enumerate(variants(mask)):
        out[k, :, :d, :h, :w] = mirror(content, m)
    return out


def unmirrored(logits, ext, mask):
    """[K, C, ed, eh, ew]: the logits [K, C, Pd, Ph, Pw] of the K variants over the real voxels, each brought back to the
    window's own orientation"""
    d, h, w = ext
    return torch.stack([mirror(logits[k, :, :d, :h, :w], m) for k, m in enumerate(variants(mask))])


def accumulate_with_map(windows, logits, mask, wmap, dt, volume, init=None):
    """(prob_sum [C, D, H, W], weight_sum [D, H, W]) in dt after the windows [(origin, extent), ..] with logits
    [K, C, Pd, Ph, Pw] each, in the kernel's order: per variant (ascending) the softmax in dt, summed, times 1 / K, times
    the weight, added; wmap: fp32 [extent] or None for weight 1.  init: accumulators to start from (not modified)."""
    n_cls = logits[0].shape[1]
    k = len(variants(mask))
    if init is None:
        psum, wsum = torch.zeros((n_cls,) + tuple(volume), dtype=dt), torch.zeros(tuple(volume), dtype=dt)
    else:
        psum, wsum = init[0].to(dt).clone(), init[1].to(dt).clone()
    for ((z, y, x), (d, h, w)), lg in zip(windows, logits):
        p = torch.zeros((n_cls, d, h, w), dtype=dt)
        for u in unmirrored(lg, (d, h, w), mask):
            p += torch.softmax(u.to(dt), 0)
        p *= 1.0 / k
        wt = torch.ones((d, h, w), dtype=dt) if wmap is None else torch.from_numpy(np.asarray(wmap)).to(dt)
        assert tuple(wt.shape) == (d, h, w)
        psum[:, z:z + d, y:y + h, x:x + w] += wt * p
        wsum[z:z + d, y:y + h, x:x + w] += wt
    return psum, wsum


def accumulate_ref(windows, logits, mask, tables, dt, volume, init=None):
    """accumulate_with_map under the map of `tables` (None: every weight 1); every window has the tables' extent"""
    return accumulate_with_map(windows, logits, mask, None if tables is None else map_of(tables), dt, volume, init)


def cal_steps(size, patch, step):
    out = []
    for s, p, st in zip(size, patch, step):
        if s <= p:
            out.append([0])
            continue
        n = int(np.ceil((s - p) / st)) + 1
        out.append([int(np.round((s - p) / (n - 1) * i)) for i in range(n)])
    return out


def predict_ref(forward, image, patch, step, importance=None, sigma_scale=1 / 8, mirror_axes=(), window_batch=4,
                dt=torch.float64):
    """The whole loop.  forward(batch [n, C, Pd, Ph, Pw] fp32) -> logits [n, n_cls, Pd, Ph, Pw], called with the batches
    sliding_window_predict forms: max(1, window_batch // K) windows, the K variants of a window side by side.  Returns
    (label uint8 [D, H, W] = argmax softmax(mean), mean = prob_sum / weight_sum, prob_sum, weight_sum), the last three in
    dt."""
    image = torch.as_tensor(image).float()
    size = tuple(image.shape[1:])
    ext = tuple(min(s, p) for s, p in zip(size, patch))
    mask = sum(1 << a for a in mirror_axes)
    k = len(variants(mask))
    wmap = importance_map(ext, sigma_scale) if importance == "gaussian" else None
    steps = cal_steps(size, patch, step)
    origins = [(z, y, x) for z in steps[0] for y in steps[1] for x in steps[2]]
    per_group = max(1, window_batch // k)
    psum = wsum = None
    for i0 in range(0, len(origins), per_group):
        group = origins[i0:i0 + per_group]
        logits = forward(torch.cat([gather_ref(image, o, ext, patch, mask) for o in group])).float().cpu()
        logits = logits.reshape((len(group), k) + tuple(logits.shape[1:]))
        init = None if psum is None else (psum, wsum)
        psum, wsum = accumulate_with_map([(o, ext) for o in group], list(logits), mask, wmap, dt, size, init)
    mean = psum / wsum
    label = torch.argmax(torch.softmax(mean, 0), 0).to(torch.uint8)
    return label, mean, psum, wsum


def check_weights(psum, wsum, extent, sigma_scale):
    """The comparison of the GPU weights test: all-zero logits of ONE class (softmax 1) accumulated into zeroed
    accumulators leave prob_sum == weight_sum == the fp32 weight, so both equal importance_map in every bit -- the floor,
    far below what any sum of weights can resolve, is visible only here"""
    want = importance_map(extent, sigma_scale).view(np.uint32)
    for name, got in (("prob_sum", psum), ("weight_sum", wsum)):
        got = got.cpu().numpy().reshape(want.shape).view(np.uint32)
        assert bool((got == want).all()), "%s differs from the importance map of %s at %g in %d of %d voxels" % (
            name, extent, sigma_scale, int((got != want).sum()), want.size)


def check_accumulators(got, ref32, ref64, init, weighted, what=""):
    """The comparison the GPU tests hold hdf_sw_accumulate_tta to.  got / ref32 / ref64: (prob_sum, weight_sum) of the
    kernel, of accumulate_ref in fp32 and in fp64; init: what the accumulators held before.  Where no window reaches
    (weight_sum's fp64 reference still at its start) both hold exactly what they held; unweighted, weight_sum is exactly the
    count; weighted, it is an fp32 sum of exact terms like prob_sum: |got - ref64| <= 4 max|ref32 - ref64| + 2^-24 |ref64|
    for every element (hip_util.check_fp32_sum).  Returns the worst error / bound of prob_sum."""
    (gp, gw), (p32, w32), (p64, w64) = got, ref32, ref64
    gp, gw = gp.cpu(), gw.cpu()
    untouched = w64 == init[1].double()
    assert torch.equal(gw[untouched], init[1][untouched]), what + ": weight_sum changed where no window reaches"
    assert torch.equal(gp[:, untouched], init[0][:, untouched]), what + ": prob_sum changed where no window reaches"
    if weighted:
        check_fp32_sum(gw, w64, 4 * float((w32.double() - w64).abs().max()), what + " weight_sum")
    else:
        assert torch.equal(gw.double(), w64), what + ": weight_sum is not the count"
    return check_fp32_sum(gp, p64, 4 * float((p32.double() - p64).abs().max()), what + " prob_sum")
