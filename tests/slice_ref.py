"""CPU restatement of slice-wise volume inference for the 2-D model (csrc/slice_infer.hip, hdf_rt.inference.slice_predict) on
top of tests/sw_ref.py: a slice of an in-plane window is a window of depth 1, so the gather and the accumulation are
sw_ref's own, called slice by slice with the mirror mask moved up by one bit (plane: bit 0 = y, 1 = x; volume: bit 0 = z, 1 =
y, 2 = x).  New in here are the per-plane normalisation in numpy fp32, the importance map of a plane -- get_gaussian((eh, ew)),
which is NOT the 3-D map of a window of depth 1: at one voxel the z table is 1 / (1 + 2 exp(-32)), not 1 -- and the loop
with the batches slice_predict forms.  torch / numpy only; tests/test_slice_ref_cpu.py pins all of it."""
import numpy as np
import torch

import sw_ref

NORM_MODE = {None: 0, "mr": 1, "max": 2}
# the cases on which the plane's map is pinned: at 1/16 every extent has zeros that the floor replaces, at 1/8 none has
EXTENTS = [(1, 7), (7, 9), (16, 16), (17, 33), (32, 48), (20, 48), (40, 64)]
SIGMA_SCALES = [1 / 8, 1 / 16]


def special_volume(seed=5, shape=(3, 5, 11, 13)):
    """fp32 [C, D, H, W] with the planes a normalisation can get wrong"""
    v = (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * 3.0).numpy()
    v[0, 1] = 0.0                                   # an all-zero plane: left alone
    v[1, 2] = -np.abs(v[1, 2]) - 0.5                # an all-negative plane: divided by a negative maximum
    v[-1, -2] = np.minimum(v[-1, -2], 1.0)
    v[-1, -2, -1, -1] = 7.5                         # the maximum is the plane's last element
    return v


def plane_max(volume):
    """[C, D]: the maximum of every plane [H, W] of a volume [C, D, H, W]"""
    return np.asarray(volume, dtype=np.float32).max(axis=(2, 3))


def normalize_planes(volume, mode):
    """fp32 [C, D, H, W].  mode 1: MRNormalize plane by plane (data_loader.py:39-50) -- divide by the plane's maximum when
    that is non-zero, one fp32 division per element, then negatives to 0; mode 2: eval.py's Normalize_2d, the same without
    the clamp; mode 0: the volume as it is"""
    v = np.array(volume, dtype=np.float32)
    if mode == 0:
        return v
    mx = plane_max(v)[:, :, None, None]
    out = np.where(mx != 0, v / np.where(mx != 0, mx, np.float32(1)), v).astype(np.float32)
    if mode == 1:
        out[out < 0] = 0
    return out


def gather_ref(volume, z0, nz, origin, ext, patch, mask, mode=0):
    """[nz, K, C, Ph, Pw]: slices outer, a slice's K variants side by side; per variant the normalised window's content
    mirrored within its clipped extent, zero-padded up to the patch at the high end of both axes"""
    v = torch.from_numpy(normalize_planes(volume, mode))
    (y0, x0), (eh, ew), (ph, pw) = origin, ext, patch
    return torch.stack([sw_ref.gather_ref(v, (z0 + s, y0, x0), (1, eh, ew), (1, ph, pw), mask << 1)[:, :, 0]
                        for s in range(nz)])


def tables_of(ext, sigma_scale):
    return tuple(sw_ref.axis_table(int(n), sigma_scale) for n in ext)


def raw_weights(tables):
    """fp32 [eh, ew]: (ty * tx) / peak in fp64, rounded once; zeros still in place"""
    ty, tx = tables
    return ((ty[:, None] * tx[None, :]) / (ty[len(ty) // 2] * tx[len(tx) // 2])).astype(np.float32)


def map_of(tables):
    """the importance map of a plane's window: zeros replaced by the smallest non-zero weight"""
    w = raw_weights(tables)
    w[w == 0] = sw_ref.floor_of(w)
    return w


def importance_map(ext, sigma_scale):
    return map_of(tables_of(ext, sigma_scale))


def accumulate_ref(z0, origin, ext, logits, mask, wmap, dt, volume, init=None):
    """(prob_sum [C, D, H, W], weight_sum [D, H, W]) in dt after the slices z0 .. of one in-plane window, logits
    [nz, K, C, Ph, Pw], in the kernel's order (sw_ref.accumulate_with_map on windows of depth 1); wmap: fp32 [eh, ew] or
    None for weight 1"""
    (y0, x0), (eh, ew) = origin, ext
    windows = [((z0 + s, y0, x0), (1, eh, ew)) for s in range(len(logits))]
    return sw_ref.accumulate_with_map(windows, [lg[:, :, None] for lg in logits], mask << 1,
                                      None if wmap is None else np.asarray(wmap)[None], dt, volume, init)


def predict_ref(forward, volume, patch, step, normalize="mr", importance=None, sigma_scale=1 / 8, mirror_axes=(),
                slice_batch=24, dt=torch.float64):
    """The whole loop.  forward(batch [n, C, Ph, Pw] fp32) -> logits [n, n_cls, Ph, Pw], called with the batches
    slice_predict forms: in-plane origins outer, slices inner in groups of max(1, slice_batch // K), a slice's K variants
    side by side.  Returns (label uint8 [D, H, W] = argmax softmax(mean), mean = prob_sum / weight_sum, prob_sum,
    weight_sum), the last three in dt."""
    volume = np.asarray(torch.as_tensor(volume).float())
    depth, plane = volume.shape[1], tuple(volume.shape[2:])
    ext = tuple(min(s, p) for s, p in zip(plane, patch))
    mask = sum(1 << a for a in mirror_axes)
    k = len(sw_ref.variants(mask << 1))
    wmap = importance_map(ext, sigma_scale) if importance == "gaussian" else None
    steps = sw_ref.cal_steps(plane, patch, step)
    per_group = max(1, slice_batch // k)
    acc = None
    for y0 in steps[0]:
        for x0 in steps[1]:
            for z0 in range(0, depth, per_group):
                nz = min(per_group, depth - z0)
                batch = gather_ref(volume, z0, nz, (y0, x0), ext, patch, mask, NORM_MODE[normalize])
                logits = forward(batch.reshape((nz * k,) + tuple(batch.shape[2:]))).float().cpu()
                logits = logits.reshape((nz, k) + tuple(logits.shape[1:]))
                acc = accumulate_ref(z0, (y0, x0), ext, logits, mask, wmap, dt, (depth,) + plane, acc)
    psum, wsum = acc
    mean = psum / wsum
    label = torch.argmax(torch.softmax(mean, 0), 0).to(torch.uint8)
    return label, mean, psum, wsum


def check_weights(psum, wsum, ext, sigma_scale):
    """sw_ref.check_weights for a plane: all-zero logits of ONE class accumulated into zeroed accumulators leave prob_sum ==
    weight_sum == the fp32 weight in every slice, so both equal importance_map in every bit, replaced zeros included"""
    want = importance_map(ext, sigma_scale).view(np.uint32)
    for name, got in (("prob_sum", psum), ("weight_sum", wsum)):
        got = got.cpu().numpy().reshape((-1,) + want.shape).view(np.uint32)
        assert bool((got == want[None]).all()), "%s differs from the importance map of %s at %g in %d of %d voxels" % (
            name, ext, sigma_scale, int((got != want[None]).sum()), got.size)
