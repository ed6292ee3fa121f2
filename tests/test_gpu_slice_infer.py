"""Slice-wise volume inference for the 2-D model (csrc/slice_infer.hip), the C entries called directly and held to
tests/slice_ref.py (itself pinned to scipy and to plain loops by tests/test_slice_ref_cpu.py):
  hdf_plane_max (one workgroup a plane)   exact on 5 planes of 7x9 (an all-zero plane, an all-negative one, a maximum in
      the last element) and on 6 planes of 384x384, from an aligned and from an unaligned start (128-bit and scalar loads);
      4100 planes, more than the grid has workgroups
  hdf_slice_gather (4096 x 256)           every element, zero padding included, for the 4 masks x 3 normalisations: slices
      1..3 of a 3 x 5 x 11x13 volume, window (2, 1), extent 7x9 in a patch 8x12 (and in 8x11, rows the 4-wide form cannot
      take); 24 slices x 4 variants x 3 channels of 64x68 and of 64x67 (past one trip of the grid in the scalar form) and of
      128x132 (past one trip in the 4-wide form)
  hdf_slice_accumulate (4096 x 256)       no tables: hdf_sw_accumulate_tta's accumulators, called slice by slice on windows
      of depth 1, in every bit (5 slices, extents 7x9 and 1x8, 2 and 8 classes, the 4 masks, three dtypes, accumulators that
      start non-zero, the voxels outside left as they were); weights: get_gaussian((eh, ew)) in every bit on 7 extents x 2
      sigma scales, replaced zeros included; weighted: within 4 max|fp32 restatement - fp64| + 2^-24 |ref| per element
      (sw_ref.check_accumulators), also on 24 slices of 150x300 = 1 080 000 voxels, past one trip of the grid
  refusals                                every one the header lists, outputs untouched
  slice_predict                           gaussian importance, both mirror axes, 'mr' on a 2 x 7 x 40x48 volume (two windows
      along y) and on its clipped part 5 x 20x48, against slice_ref.predict_ref fed by the device net itself; a plain call
      with 'max'; sliding_window_predict on the 3-D golden unchanged around them
The end-to-end input: slice_ref.predict_ref with the oracle's 2-D forward on this volume (CPU, fp64) leaves 0 of 13 440 and 0
of 4 800 voxels with two leading means closer than 4 fp32 ulp (smallest gap 3.0e-6 and 7.6e-5); the cap is 1e-3.
Worst error / bound printed on an MI355X ("ROUNDING ...", pytest -s): slice_accumulate.small f32 0.272, bf16 0.331, f16 0.276;
slice_accumulate.trip f32 0.227, bf16 0.223, f16 0.220; slice_predict.psum 0.230 (weight_sum 0.197) on the 7 x 40x48 volume,
0.225 (0.000: one window, every weight_sum a single weight) on the clipped one; slice_predict.plain 0.217; every other check
in here is exact."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import metrics_ref as mr  # noqa: E402
import slice_ref  # noqa: E402
import sw_ref  # noqa: E402
from conftest import GOLDEN  # noqa: E402
from hdf_rt._lib import BF16, F16, F32, check, lib, ptr  # noqa: E402
from hdf_rt.inference import gaussian_tables, plane_floor  # noqa: E402
from hip_util import DEV, TDT, check_fp32_sum, rnd, st  # noqa: E402

NAME = {F32: "f32", BF16: "bf16", F16: "f16"}
ALL = [F32, BF16, F16]
HDF_ERR_ARG = 1


def _bits(t):
    return t.cpu().contiguous().view(torch.int32)


def _plane_max(planes):
    """planes: device tensor [P, ...] (a view may start anywhere) -> [P] on the device, through hdf_plane_max"""
    out = torch.full((planes.shape[0],), -77.0, device=DEV)
    check(lib().hdf_plane_max(ptr(planes), planes.shape[0], planes[0].numel(), ptr(out), st()), "hdf_plane_max")
    return out


def test_plane_max_is_exact():
    v = slice_ref.special_volume()
    small = torch.from_numpy(np.stack([v[0, 1, :7, :9], v[1, 2, :7, :9], v[2, 3, 4:, 4:], v[0, 0, :7, :9], v[2, 4, :7, :9]]))
    assert float(small[0].abs().max()) == 0 and float(small[1].max()) < 0 and int(small[2].argmax()) == 62
    got = _plane_max(small.to(DEV).contiguous())
    assert torch.equal(_bits(got), _bits(small.reshape(5, -1).max(1).values))
    gen = torch.Generator().manual_seed(41)
    flat = torch.randn(6 * 384 * 384 + 1, generator=gen)
    flat[384 * 384 - 1] = 9.0                                     # the last element of the aligned plane 0
    flat[2 * 384 * 384] = 11.0                                    # the last element of the unaligned plane 1
    flat[3 * 384 * 384: 4 * 384 * 384 + 1] = -flat[3 * 384 * 384: 4 * 384 * 384 + 1].abs() - 1.0      # plane 3, either start
    dev = flat.to(DEV)
    for start in (0, 1):                                          # 16-byte aligned: 128-bit loads; off by one float: scalar
        planes = dev[start: start + 6 * 384 * 384].view(6, 384, 384)
        assert planes.data_ptr() % 16 == 4 * start
        want = flat[start: start + 6 * 384 * 384].view(6, -1).max(1).values
        assert float(want[start]) == (9.0, 11.0)[start] and float(want[3]) < 0
        assert torch.equal(_bits(_plane_max(planes)), _bits(want)), start
    # more planes than the grid has workgroups (4096): a workgroup takes a second plane
    many = torch.randn((4100, 3, 4), generator=gen)
    assert torch.equal(_bits(_plane_max(many.to(DEV))), _bits(many.reshape(4100, -1).max(1).values))


def _gather(volume, z0, nz, origin, ext, patch, mask, mode):
    k = len(sw_ref.variants(mask << 1))
    dv = torch.from_numpy(volume).to(DEV).contiguous()
    c, d = volume.shape[:2]
    pmax = _plane_max(dv.view((c * d,) + volume.shape[2:])) if mode else None
    out = torch.full((nz, k, c) + tuple(patch), -77.0, device=DEV)               # junk: every element must be written
    check(lib().hdf_slice_gather(ptr(dv), c, d, *volume.shape[2:], z0, nz, *origin, *ext, *patch, mask, mode, ptr(pmax),
                                 ptr(out), st()), "hdf_slice_gather")
    return out.cpu()


def test_gather_writes_every_element_for_every_mask_and_normalisation():
    v = slice_ref.special_volume()
    for patch in ((8, 12), (8, 11)):                                  # 8x11: a row length the 4-wide form cannot take
        for mask in range(4):
            for mode in range(3):
                got = _gather(v, 1, 3, (2, 1), (7, 9), patch, mask, mode)
                want = slice_ref.gather_ref(v, 1, 3, (2, 1), (7, 9), patch, mask, mode)
                assert torch.equal(_bits(got), _bits(want)), (patch, mask, mode)
    # past one trip of the grid: 4096 x 256 threads, four elements each where the row length is a multiple of four
    big = slice_ref.special_volume(9, (3, 24, 130, 134))
    for patch, ext, trip in (((64, 68), (61, 66), 0), ((64, 67), (61, 66), 4096 * 256), ((128, 132), (120, 131), 4 * 4096 * 256)):
        got = _gather(big, 0, 24, (5, 2), ext, patch, 3, 1)
        assert got.numel() > trip and tuple(got.shape) == (24, 4, 3) + patch
        assert torch.equal(_bits(got), _bits(slice_ref.gather_ref(big, 0, 24, (5, 2), ext, patch, 3, 1))), patch


def _accumulate(dtype, logits, mask, ext, patch, tables, acc, volume, z0, origin):
    """hdf_slice_accumulate of logits [nz, K, C, Ph, Pw] into acc = (prob_sum, weight_sum) on the device; tables: the host
    tables of the extent (gaussian_tables) or None"""
    tab, floor = None, 0.0
    if tables is not None:
        tab, floor = torch.from_numpy(np.concatenate(tables)).to(DEV), plane_floor(tables)
    dl = logits.to(DEV).to(TDT[dtype]).contiguous()
    check(lib().hdf_slice_accumulate(dtype, ptr(dl), mask, logits.shape[2], logits.shape[0], *ext, *patch, ptr(tab), floor,
                                     ptr(acc[0]), ptr(acc[1]), *volume, z0, *origin, st()), "hdf_slice_accumulate")
    return acc[0].cpu(), acc[1].cpu()


SMALL_VOLUME = (7, 11, 13)
SMALL = [((7, 9), (8, 12), (2, 1)), ((1, 8), (8, 8), (10, 2))]          # (extent, patch, origin); slices 1..5 of 7


@pytest.mark.parametrize("dtype", ALL, ids=NAME.get)
def test_without_tables_it_is_the_window_entry_slice_by_slice(dtype):
    gen = torch.Generator().manual_seed(53)
    d, h, w = SMALL_VOLUME
    for (eh, ew), (ph, pw), (y0, x0) in SMALL:
        for c in (2, 8):
            init = (torch.rand((c,) + SMALL_VOLUME, generator=gen), torch.randint(0, 3, SMALL_VOLUME, generator=gen).float())
            for mask in range(4):
                k = len(sw_ref.variants(mask << 1))
                logits = rnd(torch.randn((5, k, c, ph, pw), generator=gen) * 2.0, dtype)
                got = _accumulate(dtype, logits, mask, (eh, ew), (ph, pw), None, [t.to(DEV) for t in init], SMALL_VOLUME, 1,
                                  (y0, x0))
                want = [t.to(DEV) for t in init]
                dl = logits.to(DEV).to(TDT[dtype]).contiguous()
                per = k * c * ph * pw * dl.element_size()
                for s in range(5):
                    check(lib().hdf_sw_accumulate_tta(dtype, ptr(dl) + s * per, mask << 1, c, 1, eh, ew, 1, ph, pw, None, None,
                                                      ptr(want[0]), ptr(want[1]), d, h, w, 1 + s, y0, x0, st()),
                          "hdf_sw_accumulate_tta")
                what = ((eh, ew), c, mask)
                assert torch.equal(_bits(got[0]), _bits(want[0])) and torch.equal(_bits(got[1]), _bits(want[1])), what
                inside = torch.zeros(SMALL_VOLUME, dtype=torch.bool)
                inside[1:6, y0:y0 + eh, x0:x0 + ew] = True
                assert torch.equal(got[1][inside], init[1][inside] + 1.0), what
                assert torch.equal(got[1][~inside], init[1][~inside]) and torch.equal(got[0][:, ~inside], init[0][:, ~inside]), what
                assert not torch.equal(got[0][:, inside], init[0][:, inside])


def test_weights_are_the_reference_map_of_the_plane_bit_for_bit():
    replaced = 0
    for ext in slice_ref.EXTENTS:
        for s in slice_ref.SIGMA_SCALES:
            tables = gaussian_tables(ext, s)
            replaced += int((slice_ref.raw_weights(tables) == 0).any())
            acc = [torch.zeros((1, 2) + ext, device=DEV), torch.zeros((2,) + ext, device=DEV)]
            psum, wsum = _accumulate(F32, torch.zeros((2, 1, 1) + ext), 0, ext, ext, tables, acc, (2,) + ext, 0, (0, 0))
            slice_ref.check_weights(psum, wsum, ext, s)
    assert replaced == len(slice_ref.EXTENTS)                         # every extent at 1/16, none at 1/8


def _weighted_case(dtype, gen, nz, ext, patch, origin, volume, z0, c, mask, scale, what):
    k = len(sw_ref.variants(mask << 1))
    logits = rnd(torch.randn((nz, k, c) + patch, generator=gen) * 2.0, dtype)
    init = (torch.rand((c,) + volume, generator=gen), torch.rand(volume, generator=gen))
    wmap = slice_ref.importance_map(ext, scale)
    ref32 = slice_ref.accumulate_ref(z0, origin, ext, logits, mask, wmap, torch.float32, volume, init)
    ref64 = slice_ref.accumulate_ref(z0, origin, ext, logits, mask, wmap, torch.float64, volume, init)
    assert bool((ref64[1] == init[1].double()).any())
    got = _accumulate(dtype, logits, mask, ext, patch, gaussian_tables(ext, scale), [t.to(DEV) for t in init], volume, z0, origin)
    return sw_ref.check_accumulators(got, ref32, ref64, init, True, what)


@pytest.mark.parametrize("dtype", ALL, ids=NAME.get)
def test_weighted_accumulation_within_the_rounding_of_its_fp32_sums(dtype):
    """ROUNDING slice_accumulate (MI355X, pytest -s), worst error / bound of prob_sum: .small f32 0.272, bf16 0.331,
    f16 0.276; .trip (24 slices of 150x300, past one trip of the grid) f32 0.227, bf16 0.223, f16 0.220."""
    gen = torch.Generator().manual_seed(59)
    worst = 0.0
    for ext, patch, origin in SMALL:
        for c in (2, 8):
            for mask in range(4):
                for scale in slice_ref.SIGMA_SCALES:
                    worst = max(worst, _weighted_case(dtype, gen, 5, ext, patch, origin, SMALL_VOLUME, 1, c, mask, scale,
                                                      "%s classes %d mask %d scale %g" % (ext, c, mask, scale)))
    print("ROUNDING slice_accumulate.small %s %.3f" % (NAME[dtype], worst), flush=True)
    ext = (150, 300)
    assert 24 * ext[0] * ext[1] > 4096 * 256
    worst = _weighted_case(dtype, gen, 24, ext, (152, 304), (3, 2), (25, 154, 303), 1, 2, 2, 1 / 8, "past one trip")
    print("ROUNDING slice_accumulate.trip %s %.3f" % (NAME[dtype], worst), flush=True)


def test_bad_arguments_are_refused_before_anything_is_launched():
    ext, vol = (4, 4), (3, 4, 4)
    logits = torch.zeros((2, 1, 2) + ext, device=DEV)
    psum, wsum = torch.full((2,) + vol, 3.0, device=DEV), torch.full(vol, 2.0, device=DEV)
    tables = gaussian_tables(ext, 1 / 8)
    tab, floor = torch.from_numpy(np.concatenate(tables)).to(DEV), plane_floor(tables)
    image, pmax = torch.zeros((1,) + vol, device=DEV), torch.ones(3, device=DEV)
    out = torch.full((2, 1, 1) + ext, 9.0, device=DEV)
    big = 1 << 15

    def accumulate(n_cls=2, mask=0, nz=2, e=ext, p=ext, t=None, size=vol, z0=0, origin=(0, 0)):
        return lib().hdf_slice_accumulate(F32, ptr(logits), mask, n_cls, nz, *e, *p, ptr(t), floor, ptr(psum), ptr(wsum), *size,
                                          z0, *origin, st())

    def gather(c=1, mask=0, nz=2, e=ext, p=ext, mode=0, pm=None, size=vol, z0=0, origin=(0, 0)):
        return lib().hdf_slice_gather(ptr(image), c, *size, z0, nz, *origin, *e, *p, mask, mode, ptr(pm), ptr(out), st())

    for kw in (dict(n_cls=0), dict(n_cls=9), dict(nz=0), dict(nz=4), dict(z0=2), dict(z0=-1), dict(origin=(1, 0)),
               dict(origin=(0, -1)), dict(e=(0, 4)), dict(e=(4, 5), size=(3, 4, 5)), dict(mask=4),
               dict(e=(4000, 100), p=(4000, 100), size=(3, 4000, 100), t=tab),
               dict(nz=2, e=(big, big), p=(big, big), size=(2, big, big))):
        assert accumulate(**kw) == HDF_ERR_ARG and lib().hdf_last_error().startswith(b"slice_accumulate"), kw
    for kw in (dict(c=0), dict(nz=0), dict(nz=4), dict(z0=2), dict(origin=(1, 0)), dict(origin=(0, -1)), dict(e=(0, 4)),
               dict(e=(4, 5), size=(3, 4, 5)), dict(mask=4), dict(mode=-1), dict(mode=3, pm=pmax), dict(mode=1), dict(mode=2),
               dict(nz=2, e=(1, 1), p=(big, big))):
        assert gather(**kw) == HDF_ERR_ARG and lib().hdf_last_error().startswith(b"slice_gather"), kw
    assert lib().hdf_plane_max(ptr(image), 0, 16, ptr(pmax), st()) == HDF_ERR_ARG
    assert lib().hdf_plane_max(ptr(image), 3, 0, ptr(pmax), st()) == HDF_ERR_ARG
    torch.cuda.synchronize()
    assert float(psum.min()) == float(psum.max()) == 3.0 and float(wsum.min()) == float(wsum.max()) == 2.0
    assert float(out.min()) == float(out.max()) == 9.0 and float(pmax.min()) == float(pmax.max()) == 1.0
    assert accumulate(t=tab) == 0 and gather(mode=1, pm=pmax) == 0                # and the good calls go through
    assert lib().hdf_plane_max(ptr(image), 3, 16, ptr(pmax), st()) == 0


def _leading_means(psum64, wsum64):
    """(first argmax of prob_sum / weight_sum in fp64, excluded: the two leading means differ by less than 4 fp32 ulp)"""
    mean = psum64 / wsum64
    top2 = mean.topk(2, 0).values
    gap = top2[0] - top2[1]
    ulp = torch.exp2(torch.floor(torch.log2(top2[0].clamp_min(1e-300))) - 23)
    return mr.first_argmax(mean, 0), (gap > 0) & (gap < 4 * ulp)


def _golden_3d():
    from models.HDenseFormer import HDenseFormer
    from oracle import detgen
    from oracle import hdf_oracle as orc
    g = np.load(os.path.join(GOLDEN, "g8_sliding_window.npz"), allow_pickle=False)
    in_ch, n_cls, nf, td = [int(v) for v in g["cfg"]]
    patch, step = tuple(int(v) for v in g["patch"]), tuple(int(v) for v in g["step"])
    net = HDenseFormer(in_ch, n_cls, nf, image_size=patch, transformer_depth=td)
    net.load_state_dict(orc.det_model(in_ch, n_cls, nf, patch, td))
    net = net.cuda().eval()
    net.compute_dtype = "fp32"
    image = torch.from_numpy(detgen.det_input(1, in_ch, tuple(int(v) for v in g["image_size"]), tag="sw")[0])
    return net, image, patch, step


def test_slice_predict_end_to_end():
    """ROUNDING slice_predict.psum (MI355X, pytest -s): 0.230 of the bound on the 7 x 40x48 volume (weight_sum 0.197), 0.225
    (0.000) on the clipped 5 x 20x48 one; slice_predict.plain 0.217; no label differed outside the excluded voxels, and
    none was excluded."""
    from hdf_rt import inference
    from models.HDenseFormer_2D import HDenseFormer_2D
    from oracle import detgen
    from oracle import hdf_oracle as orc
    net3, image3, patch3, step3 = _golden_3d()
    before = inference.sliding_window_predict(net3, image3, patch3, step3, return_probabilities=True)
    patch, step = (32, 48), (16, 24)
    net = HDenseFormer_2D(2, 2, 16, image_size=patch, transformer_depth=4)
    net.load_state_dict(orc.det_model(2, 2, 16, patch, 4))
    net = net.cuda().train()
    net.compute_dtype = "fp32"
    full = torch.from_numpy(detgen.det_input(1, 2, (7, 40, 48), tag="slice")[0])
    answers = []

    def device_net(batch):
        with torch.no_grad():
            answers.append(net(batch.to(DEV))[0].float().cpu())
        return answers[-1]

    opts = dict(importance="gaussian", mirror_axes=(0, 1), normalize="mr")
    for volume in (full, full[:, :5, :20]):
        lab, mean = inference.slice_predict(net, volume, 8, step_size=step, return_probabilities=True, **opts)
        assert net.training                                                           # restored
        psum, wsum = inference._slice_sums(net, volume, 8, "mr", step, "gaussian", 1 / 8, (0, 1))
        assert torch.equal(mean, psum / wsum) and tuple(lab.shape) == tuple(volume.shape[1:]) and lab.dtype == torch.uint8
        assert lab.device == psum.device == next(net.parameters()).device
        net.eval()
        del answers[:]
        _, _, p64, w64 = slice_ref.predict_ref(device_net, volume, patch, step, slice_batch=8, dt=torch.float64, **opts)
        replay = iter(list(answers))                                                  # the same answers, accumulated in fp32
        _, _, p32, w32 = slice_ref.predict_ref(lambda batch: next(replay), volume, patch, step, slice_batch=8,
                                               dt=torch.float32, **opts)
        net.train()
        windows = 2 if volume.shape[2] > patch[0] else 1
        assert [a.shape[0] for a in answers] == ([8] * ((volume.shape[1] - 1) // 2) + [4]) * windows
        assert answers[0].shape[0] == 8                                               # 2 slices x 4 variants a forward
        worst_w = check_fp32_sum(wsum.cpu(), w64, 4 * float((w32.double() - w64).abs().max()), "weight_sum")
        worst_p = check_fp32_sum(psum.cpu(), p64, 4 * float((p32.double() - p64).abs().max()), "prob_sum")
        print("ROUNDING slice_predict.psum %s %.3f wsum %.3f" % (tuple(volume.shape[1:]), worst_p, worst_w), flush=True)
        want, excluded = _leading_means(p64, w64)
        assert float(excluded.double().mean()) <= 1e-3
        got = lab.cpu().long()
        assert torch.equal(got[~excluded], want[~excluded]), int((got != want)[~excluded].sum())
    # a plain call, eval.py:208-230: every slice divided by its planes' maxima, one forward of all five, the softmax
    net.eval()
    volume = full[:, :5, :32].contiguous()
    lab, prob = inference.slice_predict(net, volume.numpy(), normalize="max", return_probabilities=True)
    slices = torch.from_numpy(slice_ref.normalize_planes(volume.numpy(), 2)).permute(1, 0, 2, 3).contiguous()
    with torch.no_grad():
        logits = net(slices.to(DEV))[0].float().cpu()[:, None]                         # [5, 1, n_cls, 32, 48]
    ref32 = slice_ref.accumulate_ref(0, (0, 0), patch, logits, 0, None, torch.float32, (5,) + patch)
    ref64 = slice_ref.accumulate_ref(0, (0, 0), patch, logits, 0, None, torch.float64, (5,) + patch)
    assert torch.equal(ref64[1], torch.ones((5,) + patch, dtype=torch.float64))
    worst = check_fp32_sum(prob.cpu(), ref64[0], 4 * float((ref32[0].double() - ref64[0]).abs().max()), "probabilities")
    print("ROUNDING slice_predict.plain %.3f" % worst, flush=True)
    want, excluded = _leading_means(*ref64)
    assert float(excluded.double().mean()) <= 1e-3
    assert torch.equal(lab.cpu().long()[~excluded], want[~excluded])
    after = inference.sliding_window_predict(net3, image3, patch3, step3, return_probabilities=True)
    assert torch.equal(before[0], after[0]) and torch.equal(_bits(before[1]), _bits(after[1]))
