"""tests/sw_ref.py, the CPU restatement that tests/test_gpu_sw_tta.py holds csrc/sw_infer.hip to, checked on its own ground:
  - its importance map and hdf_rt.inference.gaussian_tables equal the reference's get_gaussian (trainer.py:620-638) --
    scipy.ndimage.gaussian_filter of a unit impulse at n // 2, mode='constant', divided by its maximum, cast to fp32, zeros
    replaced by the smallest non-zero -- in every bit, on 10 extents x 4 sigma scales; zero replacement and the fp32
    denormal occur among them;
  - with no importance and no mirroring the loop is oracle.sw_oracle.sliding_window exactly;
  - mirroring changes nothing for a net that is pointwise in the voxel, and equals a torch.flip average for one that is not;
  - the comparison the GPU test uses (sw_ref.check_accumulators, torch.equal for the gather) rejects six planted defects."""
import numpy as np
import pytest
import torch

import sw_ref
from hdf_rt.inference import gaussian_tables
from oracle import sw_oracle

CASES = [(e, s) for e in sw_ref.EXTENTS for s in sw_ref.SIGMA_SCALES]


def _scipy_map(extent, sigma_scale):
    """get_gaussian as the reference writes it; returns (map, number of zeros replaced)"""
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


def test_importance_map_is_scipy_gaussian_filter_bit_for_bit():
    replaced, denormal = {s: 0 for s in sw_ref.SIGMA_SCALES}, 0
    for extent, s in CASES:
        want, zeros = _scipy_map(extent, s)
        assert _same_bits(sw_ref.importance_map(extent, s), want), (extent, s)
        tables = gaussian_tables(extent, s)
        assert all(t.dtype == np.float64 and t.shape == (n,) for t, n in zip(tables, extent))
        for t, r in zip(tables, sw_ref.tables_of(extent, s)):
            assert bool((t.view(np.uint64) == r.view(np.uint64)).all()), (extent, s)
        assert _same_bits(sw_ref.map_of(tables), want), (extent, s)
        assert zeros == int((sw_ref.raw_weights(tables) == 0).sum())
        replaced[s] += zeros > 0
        tiny = np.float32(2.0) ** -126
        denormal += bool(((want > 0) & (want < tiny)).any())
    # scipy's own map has zeros to replace in eight of the ten extents at 1/16 (not (2, 2, 2), the denormal case, nor
    # (1, 1, 1)) and in nine at 1/32 (not (1, 1, 1)), nowhere at 1/8 and 1/4: 17 of the 40 cases
    assert replaced == {1 / 8: 0, 1 / 4: 0, 1 / 16: 8, 1 / 32: 9} and denormal >= 1, (replaced, denormal)
    two = sw_ref.importance_map((2, 2, 2), 1 / 16)
    assert 0 < float(two.min()) < 2.0 ** -126 and int((sw_ref.raw_weights(sw_ref.tables_of((2, 2, 2), 1 / 16)) == 0).sum()) == 0


def test_gaussian_tables_defaults_and_errors():
    for a, b in zip(gaussian_tables((7, 9, 5)), sw_ref.tables_of((7, 9, 5), 1 / 8)):
        assert np.array_equal(a, b)
    with pytest.raises(ValueError):
        gaussian_tables((0, 4, 4))
    with pytest.raises(ValueError):
        gaussian_tables((4, 4, 4), 0.0)


def test_predict_options_are_validated_before_anything_runs():
    from hdf_rt.inference import sliding_window_predict
    for kw in ({"importance": "linear"}, {"mirror_axes": (3,)}, {"mirror_axes": (0, 0)}, {"mirror_axes": (-1,)},
               {"mirror_axes": (1.0,)}):
        with pytest.raises(ValueError):
            sliding_window_predict(None, None, (8, 8, 8), (4, 4, 4), **kw)


# a small volume, clipped along z (6 < 8) and walked along y and x
PATCH, STEP, N_CLS = (8, 8, 8), (4, 4, 4), 3


def _image(seed=11, size=(6, 13, 11)):
    return torch.randn((2,) + size, generator=torch.Generator().manual_seed(seed))


def _pointwise(p):
    """[n, 2, ...] -> [n, 3, ...]: one correctly rounded operation per element, the same on any layout"""
    return torch.stack([p[:, 0] - p[:, 1], p[:, 0] * 2.0, p[:, 1] * -0.5], 1)


def _with_ramp(p):
    """not pointwise: the answer depends on where along x of the patch a voxel sits"""
    ramp = torch.arange(p.shape[-1], dtype=p.dtype) * 0.25
    out = _pointwise(p)
    out[:, 0] += ramp
    out[:, 2] -= ramp * ramp * 0.125
    return out


def test_plain_loop_is_the_oracle_exactly():
    image = _image()
    lab, mean, _, wsum = sw_ref.predict_ref(_pointwise, image, PATCH, STEP, dt=torch.float32)
    want_lab, want_mean = sw_oracle.sliding_window(_pointwise, image, N_CLS, PATCH, STEP)
    assert float(wsum.max()) > 1 and image.shape[1] < PATCH[0]
    assert np.array_equal(lab.numpy(), want_lab)
    assert np.array_equal(mean.numpy(), want_mean)


@pytest.mark.parametrize("importance", [None, "gaussian"])
def test_mirroring_leaves_a_pointwise_net_alone(importance):
    image = _image(12)
    _, mean0, p0, w0 = sw_ref.predict_ref(_pointwise, image, PATCH, STEP, importance=importance)
    for axes in [(0,), (1, 2), (0, 1, 2)]:
        _, mean, p, w = sw_ref.predict_ref(_pointwise, image, PATCH, STEP, importance=importance, mirror_axes=axes)
        assert torch.equal(w, w0)
        assert float((p - p0).abs().max()) <= 8 * 2.0 ** -52 * float(p0.abs().max())     # K fp64 additions and a product
        assert float((mean - mean0).abs().max()) <= 16 * 2.0 ** -52


def test_mirroring_a_net_with_a_ramp_is_the_flip_average():
    image = _image(13)
    size = tuple(image.shape[1:])
    ext = tuple(min(s, p) for s, p in zip(size, PATCH))
    for axes in [(2,), (0, 2), (0, 1, 2)]:
        _, mean, psum, wsum = sw_ref.predict_ref(_with_ramp, image, PATCH, STEP, importance="gaussian", mirror_axes=axes,
                                                window_batch=1)
        wmap = torch.from_numpy(sw_ref.importance_map(ext, 1 / 8)).double()
        want_p, want_w = torch.zeros((N_CLS,) + size, dtype=torch.float64), torch.zeros(size, dtype=torch.float64)
        steps = sw_ref.cal_steps(size, PATCH, STEP)
        subsets = [[a for i, a in enumerate(axes) if bits >> i & 1] for bits in range(1 << len(axes))]
        for z in steps[0]:
            for y in steps[1]:
                for x in steps[2]:
                    content = image[:, z:z + ext[0], y:y + ext[1], x:x + ext[2]]
                    prob = torch.zeros((N_CLS,) + ext, dtype=torch.float64)
                    for sub in subsets:
                        dims = [1 + a for a in sub]
                        padded = torch.zeros((1, 2) + PATCH)
                        padded[0, :, :ext[0], :ext[1], :ext[2]] = torch.flip(content, dims) if dims else content
                        lg = _with_ramp(padded)[0, :, :ext[0], :ext[1], :ext[2]]
                        sm = torch.softmax(lg.double(), 0)
                        prob += torch.flip(sm, dims) if dims else sm
                    want_p[:, z:z + ext[0], y:y + ext[1], x:x + ext[2]] += wmap * (prob / len(subsets))
                    want_w[z:z + ext[0], y:y + ext[1], x:x + ext[2]] += wmap
        assert torch.equal(wsum, want_w)
        assert float((psum - want_p).abs().max()) <= 1e-14
        # and the ramp matters: without mirroring the answer is another one
        _, _, plain, _ = sw_ref.predict_ref(_with_ramp, image, PATCH, STEP, importance="gaussian", window_batch=1)
        assert float((plain - psum).abs().max()) > 1e-3


# ------------------------------------------------------------------------------------------ planted defects
VOLUME = (9, 10, 9)
WINDOWS = [((0, 0, 0), (6, 6, 6)), ((3, 4, 2), (6, 6, 6)), ((1, 2, 3), (6, 6, 6))]      # (8, 9, 8) is never reached
PPATCH = (8, 8, 8)


def _logits(mask, seed=21, n_cls=3):
    gen = torch.Generator().manual_seed(seed)
    k = len(sw_ref.variants(mask))
    return [torch.randn((k, n_cls) + PPATCH, generator=gen) * 2.0 for _ in WINDOWS]


def _init(n_cls=3, seed=22):
    gen = torch.Generator().manual_seed(seed)
    return torch.rand((n_cls,) + VOLUME, generator=gen), torch.randint(0, 3, VOLUME, generator=gen).float()


def _check(got, logits, mask, tables, init):
    ref32 = sw_ref.accumulate_ref(WINDOWS, logits, mask, tables, torch.float32, VOLUME, init)
    ref64 = sw_ref.accumulate_ref(WINDOWS, logits, mask, tables, torch.float64, VOLUME, init)
    return sw_ref.check_accumulators(got, ref32, ref64, init, tables is not None, "planted")


def _fp32(logits, mask, wmap, init):
    return sw_ref.accumulate_with_map(WINDOWS, logits, mask, wmap, torch.float32, VOLUME, init)


def test_the_comparison_accepts_the_fp32_restatement():
    init = _init()
    for mask in (0, 0b101, 0b111):
        for tables in (None, sw_ref.tables_of((6, 6, 6), 1 / 8), sw_ref.tables_of((6, 6, 6), 1 / 16)):
            lg = _logits(mask)
            wmap = None if tables is None else sw_ref.map_of(tables)
            assert _check(_fp32(lg, mask, wmap, init), lg, mask, tables, init) <= 0.25


def test_the_comparison_rejects_planted_defects():
    init = _init()
    t8, t16 = sw_ref.tables_of((6, 6, 6), 1 / 8), sw_ref.tables_of((6, 6, 6), 1 / 16)
    assert int((sw_ref.raw_weights(t16) == 0).sum()) > 0
    # 1. un-mirroring along the wrong axis: variants made for a z mirror, brought back along y
    lg = _logits(0b001)
    with pytest.raises(AssertionError):
        _check(_fp32(lg, 0b010, sw_ref.map_of(t8), init), lg, 0b001, t8, init)
    # 3. the weight applied to prob_sum but not to weight_sum
    lg = _logits(0b101)
    psum, _ = _fp32(lg, 0b101, sw_ref.map_of(t8), init)
    _, count = _fp32(lg, 0b101, None, init)
    with pytest.raises(AssertionError):
        _check((psum, count), lg, 0b101, t8, init)
    # 4. the centre at (n - 1) // 2: on an even axis the map moves by one voxel
    shifted = tuple(sw_ref.axis_table(6, 1 / 8, centre=(6 - 1) // 2) for _ in range(3))
    with pytest.raises(AssertionError):
        _check(_fp32(lg, 0b101, sw_ref.map_of(shifted), init), lg, 0b101, t8, init)
    # 5. the floor not applied: zeros left in the map.  The floor is far below what a sum of weights near 1 resolves,
    # so it is the weights test's comparison -- bit equality on zeroed accumulators -- that sees it
    raw = torch.from_numpy(sw_ref.raw_weights(t16))
    with pytest.raises(AssertionError):
        sw_ref.check_weights(raw, raw, (6, 6, 6), 1 / 16)
    good = torch.from_numpy(sw_ref.map_of(t16))
    sw_ref.check_weights(good, good, (6, 6, 6), 1 / 16)
    with pytest.raises(AssertionError):                              # (and defect 4 once more)
        sw_ref.check_weights(torch.from_numpy(sw_ref.map_of(shifted)), good, (6, 6, 6), 1 / 8)
    # 6. averaging the logits instead of the softmaxes
    mean_logits = [sw_ref.unmirrored(l, (6, 6, 6), 0b101).mean(0, keepdim=True) for l in lg]
    with pytest.raises(AssertionError):
        _check(_fp32(mean_logits, 0, sw_ref.map_of(t8), init), lg, 0b101, t8, init)


def test_equality_rejects_a_gather_that_flips_the_padded_patch():
    # 2. flipping the padded patch instead of the content: the zeros move to the low end of a clipped, mirrored axis
    image = _image(14, (11, 13, 9))
    origin, ext, patch = (2, 3, 1), (7, 9, 5), (8, 12, 8)
    for mask in range(1, 8):
        want = sw_ref.gather_ref(image, origin, ext, patch, mask)
        plain = sw_ref.gather_ref(image, origin, ext, patch, 0)[0]
        bad = torch.stack([sw_ref.mirror(plain, m) for m in sw_ref.variants(mask)])
        assert bad.shape == want.shape and not torch.equal(bad, want)
        assert torch.equal(bad[0], want[0])                       # variant 0 is the window itself either way
