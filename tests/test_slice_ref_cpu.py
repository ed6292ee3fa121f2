"""tests/slice_ref.py, the CPU restatement that tests/test_gpu_slice_infer.py holds csrc/slice_infer.hip to, checked on its
own ground:
  - the plane's importance map, hdf_rt.inference.gaussian_tables((eh, ew)) and plane_floor equal the reference's
    get_gaussian((eh, ew)) (trainer.py:620-638: scipy.ndimage.gaussian_filter of a unit impulse, over its maximum, cast to
    fp32, zeros replaced by the smallest non-zero) in every bit on 7 extents x 2 sigma scales; at 1/16 every extent has
    zeros to replace, at 1/8 none;
  - the normalisation equals a plain loop over the planes (data_loader.py:39-50, eval.py:112-123) on a volume with an
    all-zero plane, an all-negative plane and a plane whose maximum is its last element;
  - the loop equals a plain loop over slices for a per-pixel linear "net", and mirroring leaves such a net alone;
  - the comparisons the GPU tests use (torch.equal for the gather, sw_ref.check_accumulators, slice_ref.check_weights)
    reject six planted defects."""
import numpy as np
import pytest
import torch

import slice_ref
import sw_ref
from hdf_rt.inference import gaussian_tables, plane_floor

CASES = [(e, s) for e in slice_ref.EXTENTS for s in slice_ref.SIGMA_SCALES]


def _scipy_map(extent, sigma_scale):
    """get_gaussian as the reference writes it, on a plane; returns (map, number of zeros replaced)"""
    from scipy.ndimage import gaussian_filter
    tmp = np.zeros(extent)
    tmp[tuple(i // 2 for i in extent)] = 1
    g = gaussian_filter(tmp, [i * sigma_scale for i in extent], 0, mode='constant', cval=0)
    g = (g / np.max(g) * 1).astype(np.float32)
    zeros = int((g == 0).sum())
    g[g == 0] = np.min(g[g != 0])
    return g, zeros


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


def test_plane_map_is_scipy_gaussian_filter_bit_for_bit():
    replaced = {s: 0 for s in slice_ref.SIGMA_SCALES}
    for extent, s in CASES:
        want, zeros = _scipy_map(extent, s)
        assert _same_bits(slice_ref.importance_map(extent, s), want), (extent, s)
        tables = gaussian_tables(extent, s)
        assert len(tables) == 2 and all(t.dtype == np.float64 and t.shape == (n,) for t, n in zip(tables, extent))
        for t, r in zip(tables, slice_ref.tables_of(extent, s)):
            assert bool((t.view(np.uint64) == r.view(np.uint64)).all()), (extent, s)
        raw = slice_ref.raw_weights(tables)
        assert zeros == int((raw == 0).sum())
        # the floor the host hands to hdf_slice_accumulate is the value scipy's map carries in the replaced places
        floor = np.float32(plane_floor(tables))
        assert floor.view(np.uint32) == want.min().view(np.uint32) and float(floor) == plane_floor(tables)
        raw[raw == 0] = floor
        assert _same_bits(raw, want), (extent, s)
        replaced[s] += zeros > 0
    assert replaced == {1 / 8: 0, 1 / 16: len(slice_ref.EXTENTS)}, replaced


def test_the_plane_map_is_not_the_volume_map_of_depth_one():
    # why the slice entries carry two tables of their own: one voxel along z leaves 1 / (1 + 2 exp(-32)) in tz, not 1
    two = slice_ref.raw_weights(slice_ref.tables_of((7, 9), 1 / 8))
    three = sw_ref.raw_weights(sw_ref.tables_of((1, 7, 9), 1 / 8))[0]
    assert sw_ref.axis_table(1, 1 / 8)[0] < 1.0
    assert two.shape == three.shape and float(np.abs(two.astype(np.float64) - three).max()) <= 2.0 ** -24


_volume = slice_ref.special_volume


def _loop_normalize(volume, clamp):
    out = volume.copy()
    for c in range(out.shape[0]):                   # eval.py:117-120 / data_loader.py:43-47, plane by plane
        for z in range(out.shape[1]):
            if np.max(out[c, z]) != 0:
                out[c, z] = out[c, z] / np.max(out[c, z])
    if clamp:
        out[out < 0] = 0
    return out


def test_normalisation_is_the_plain_loop_over_planes():
    v = _volume()
    assert float(v[0, 1].max()) == 0 and float(v[1, 2].max()) < 0 and int(v[2, 3].argmax()) == v[2, 3].size - 1
    assert _same_bits(slice_ref.normalize_planes(v, 0), v)
    assert _same_bits(slice_ref.normalize_planes(v, 1), _loop_normalize(v, True))
    assert _same_bits(slice_ref.normalize_planes(v, 2), _loop_normalize(v, False))
    mr, mx = slice_ref.normalize_planes(v, 1), slice_ref.normalize_planes(v, 2)
    assert float(mr.min()) == 0 and float(mx.min()) < 0 and float(mr[2].max()) == float(mx[2].max()) == 1
    assert float(mx[1, 2].min()) == 1.0             # negative / negative maximum: the plane turns positive, at least 1
    assert not slice_ref.normalize_planes(v, 1) is v and float(v[2, 3, -1, -1]) == 7.5       # the input is not modified


def test_predict_options_are_validated_before_anything_runs():
    from hdf_rt.inference import slice_predict
    for kw in ({"importance": "linear"}, {"mirror_axes": (2,)}, {"mirror_axes": (0, 0)}, {"mirror_axes": (-1,)},
               {"mirror_axes": (1.0,)}, {"normalize": "petct"}, {}):
        with pytest.raises(ValueError):
            slice_predict(None, None, **kw)
    with pytest.raises(ValueError, match="HDenseFormer_2D"):
        from models.HDenseFormer import HDenseFormer_16
        slice_predict(HDenseFormer_16(2, 3, (32, 32, 32), 8), np.zeros((2, 4, 32, 32), np.float32))
    import hdf_rt
    assert hdf_rt.slice_predict is slice_predict and "slice_predict" in dir(hdf_rt)


PATCH, STEP, N_CLS = (8, 8), (4, 4), 3


def _pointwise(p):
    """[n, 2, H, W] -> [n, 3, H, W]: per pixel and linear, one correctly rounded operation per element: it commutes with
    mirroring"""
    return torch.stack([p[:, 0] - p[:, 1], p[:, 0] * 2.0, p[:, 1] * -0.5], 1)


@pytest.mark.parametrize("normalize", [None, "mr", "max"])
def test_the_loop_is_a_plain_loop_over_slices(normalize):
    v = _volume(6, (2, 5, 6, 13))                                   # clipped along y (6 < 8), walked along x
    forwards = []

    def net(batch):
        forwards.append(batch.shape[0])
        return _pointwise(batch)

    lab, mean, psum, wsum = slice_ref.predict_ref(net, v, PATCH, STEP, normalize=normalize, slice_batch=2)
    xs = sw_ref.cal_steps((6, 13), PATCH, STEP)[1]
    assert len(xs) == 3 and forwards == [2, 2, 1] * 3                # origins outer, slices in groups of two
    vn = torch.from_numpy(_loop_normalize(v, normalize == "mr") if normalize else v)
    want_p, want_w = torch.zeros((N_CLS, 5, 6, 13), dtype=torch.float64), torch.zeros((5, 6, 13), dtype=torch.float64)
    for x0 in xs:
        for z in range(5):
            padded = torch.zeros((1, 2) + PATCH)
            padded[0, :, :6] = vn[:, z, :, x0:x0 + 8]
            want_p[:, z, :, x0:x0 + 8] += torch.softmax(_pointwise(padded)[0, :, :6].double(), 0)
            want_w[z, :, x0:x0 + 8] += 1
    assert torch.equal(wsum, want_w) and float(wsum.max()) > 1
    assert float((psum - want_p).abs().max()) <= 4 * 2.0 ** -52 * float(want_p.max())
    assert torch.equal(lab.long(), torch.argmax(torch.softmax(mean, 0), 0))


@pytest.mark.parametrize("importance", [None, "gaussian"])
def test_mirroring_leaves_a_pointwise_net_alone(importance):
    v = _volume(7, (2, 3, 6, 13))
    _, mean0, p0, w0 = slice_ref.predict_ref(_pointwise, v, PATCH, STEP, importance=importance, slice_batch=4)
    for axes in [(0,), (1,), (0, 1)]:
        forwards = []

        def net(batch):
            forwards.append(batch.shape[0])
            return _pointwise(batch)

        _, mean, p, w = slice_ref.predict_ref(net, v, PATCH, STEP, importance=importance, mirror_axes=axes, slice_batch=4)
        k = 1 << len(axes)
        assert forwards[0] == 4 // k * k and torch.equal(w, w0)
        assert float((p - p0).abs().max()) <= 8 * 2.0 ** -52 * float(p0.abs().max())     # K fp64 additions and a product
        assert float((mean - mean0).abs().max()) <= 16 * 2.0 ** -52


# ------------------------------------------------------------------------------------------ planted defects
ORIGIN, EXT, GPATCH = (2, 1), (7, 9), (8, 12)


def test_equality_rejects_four_planted_gather_defects():
    v = _volume()
    want = {(mask, mode): slice_ref.gather_ref(v, 1, 3, ORIGIN, EXT, GPATCH, mask, mode) for mask in range(4) for mode in range(3)}
    assert tuple(want[3, 1].shape) == (3, 4, 3, 8, 12)
    for mask in range(1, 4):
        # 1. the padded patch flipped instead of the content: the zeros move to the low end of a mirrored axis
        plain = want[0, 1][:, 0]
        bad = torch.stack([torch.stack([sw_ref.mirror(plain[s], m << 1) for m in range(4) if m & ~mask == 0])
                           for s in range(3)])
        assert bad.shape == want[mask, 1].shape and not torch.equal(bad, want[mask, 1])
        assert torch.equal(bad[:, 0], want[mask, 1][:, 0])           # variant 0 is the window itself either way
    # 3. the variants out of order (descending code)
    assert not torch.equal(torch.flip(want[3, 1], [1]), want[3, 1])
    for mode in (1, 2):
        # 2. the maximum of the window instead of the plane's: plane (2, 3) has its maximum outside the window
        window = v[:, :, ORIGIN[0]:ORIGIN[0] + EXT[0], ORIGIN[1]:ORIGIN[1] + EXT[1]]
        wmax = window.max(axis=(2, 3))[:, :, None, None]
        local = np.where(wmax != 0, v / np.where(wmax != 0, wmax, 1), v).astype(np.float32)
        if mode == 1:
            local[local < 0] = 0
        bad = slice_ref.gather_ref(local, 1, 3, ORIGIN, EXT, GPATCH, 0, 0)
        assert not torch.equal(bad, want[0, mode]) and not torch.equal(bad[2, 0, 2], want[0, mode][2, 0, 2])
        # 6. the channel's maximum over the volume instead of the plane's
        cmax = v.max(axis=(1, 2, 3))[:, None, None, None]
        local = (v / cmax).astype(np.float32)
        if mode == 1:
            local[local < 0] = 0
        assert not torch.equal(slice_ref.gather_ref(local, 1, 3, ORIGIN, EXT, GPATCH, 0, 0), want[0, mode])
    # 4. the clamp before the division: the all-negative plane (1, 2) becomes 0 instead of positive
    early = np.maximum(v, 0)
    bad = slice_ref.gather_ref(early, 1, 3, ORIGIN, EXT, GPATCH, 0, 2)
    assert not torch.equal(bad, want[0, 1]) and float(bad[1, 0, 1].abs().max()) == 0 and float(want[0, 1][1, 0, 1].max()) >= 1


VOLUME = (4, 10, 12)


def _accumulate_case(mask, weighted, seed=23, scale=1 / 8):
    gen = torch.Generator().manual_seed(seed)
    k = len(sw_ref.variants(mask << 1))
    logits = torch.randn((3, k, N_CLS) + GPATCH, generator=gen) * 2.0
    init = torch.rand((N_CLS,) + VOLUME, generator=gen), torch.randint(0, 3, VOLUME, generator=gen).float()
    wmap = slice_ref.importance_map(EXT, scale) if weighted else None
    ref = [slice_ref.accumulate_ref(1, ORIGIN, EXT, logits, mask, wmap, dt, VOLUME, init) for dt in (torch.float32, torch.float64)]
    return logits, init, wmap, ref


def test_the_comparison_accepts_the_fp32_restatement():
    for mask in range(4):
        for weighted in (False, True):
            _, init, _, (ref32, ref64) = _accumulate_case(mask, weighted)
            assert bool((ref64[1] == init[1].double()).any())         # slice 0 and the plane's border are never reached
            assert sw_ref.check_accumulators(ref32, ref32, ref64, init, weighted, "fp32") <= 0.25


def test_the_comparisons_reject_planted_accumulation_defects():
    # 3. (once more, in the tail) the variants brought back in descending order
    logits, init, wmap, (ref32, ref64) = _accumulate_case(3, True)
    bad = slice_ref.accumulate_ref(1, ORIGIN, EXT, torch.flip(logits, [1]), 3, wmap, torch.float32, VOLUME, init)
    with pytest.raises(AssertionError):
        sw_ref.check_accumulators(bad, ref32, ref64, init, True, "planted")
    # the map of the depth-1 volume window in the place of the plane's is NOT a defect this bound resolves (one ulp of the
    # weight); a slice too many is
    bad = slice_ref.accumulate_ref(0, ORIGIN, EXT, logits, 3, wmap, torch.float32, VOLUME, init)
    with pytest.raises(AssertionError):
        sw_ref.check_accumulators(bad, ref32, ref64, init, True, "planted")
    # 5. the floor omitted: zeros left in the map.  Far below what a sum of weights near 1 resolves, so it is the weights
    # test's comparison -- bit equality on zeroed accumulators -- that sees it
    for ext in slice_ref.EXTENTS:
        tables = slice_ref.tables_of(ext, 1 / 16)
        raw = torch.from_numpy(slice_ref.raw_weights(tables))
        assert int((raw == 0).sum()) > 0
        with pytest.raises(AssertionError):
            slice_ref.check_weights(raw.expand(2, *ext), raw.expand(2, *ext), ext, 1 / 16)
        good = torch.from_numpy(slice_ref.map_of(tables)).expand(2, *ext)
        slice_ref.check_weights(good, good, ext, 1 / 16)
