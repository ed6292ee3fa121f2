"""Sliding-window inference with a Gaussian importance map and mirror test-time augmentation (csrc/sw_infer.hip), the C
entries called directly and held to tests/sw_ref.py (itself pinned to scipy and to the oracle by tests/test_sw_ref_cpu.py):
  hdf_sw_gather (4096 x 256)            every element, zero padding included, for all 8 masks: extent 7x9x5 in a patch 8x12x8
      at (2, 3, 1) of an 11x13x9 volume (and in 8x12x7, rows the 4-wide form cannot take); 8 x 2 x 64x64x68 and
      8 x 2 x 40x44x50 elements, past one trip of the grid in either form
  hdf_sw_importance_floor, weights      zero logits of one class into zeroed accumulators leave prob_sum == weight_sum == w:
      both equal get_gaussian's map in every bit on 10 extents x 4 sigma scales (zeros replaced in 17 of them, one fp32
      denormal), and so does the floor
  hdf_sw_accumulate_tta (4096 x 256)    mask 0, no tables, patch == extent: hdf_sw_accumulate's accumulators in every bit;
      window 96x104x112 = 1 118 208 voxels in a 100x110x120 volume, mask 0b101, weighted, five windows (one clipped, with
      its own tables); extents 7x9x5 and 1x8x8 under all 8 masks, weighted or not, 2 and 8 classes, accumulators that start
      non-zero.  Untouched voxels exact, unweighted weight_sum exact, prob_sum (and weighted weight_sum) per element within
      4 max|fp32 restatement - fp64| + 2^-24 |ref| (sw_ref.check_accumulators)
  sliding_window_predict                importance='gaussian', mirror_axes=(0, 2) on the golden's model and image against
      sw_ref.predict_ref fed by the device net itself; once more with a clipped axis; the default call unchanged around them
Worst error / bound printed on an MI355X ("ROUNDING ...", pytest -s): sw_accumulate_tta.psum f32 0.226, bf16 0.226,
f16 0.224; sw_accumulate_tta.small f32 0.306, bf16 0.269, f16 0.296; sw_predict_tta.psum 0.229 (weight_sum 0.227) on the
whole image, 0.218 (0.197) on the clipped one; every other check in here is exact."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import metrics_ref as mr  # noqa: E402
import sw_ref  # noqa: E402
from conftest import GOLDEN  # noqa: E402
from hdf_rt._lib import BF16, F16, F32, check, lib, ptr  # noqa: E402
from hip_util import DEV, TDT, check_fp32_sum, rnd, st  # noqa: E402

NAME = {F32: "f32", BF16: "bf16", F16: "f16"}
ALL = [F32, BF16, F16]
HDF_ERR_ARG = 1


def _gather(image, origin, ext, patch, mask):
    k = len(sw_ref.variants(mask))
    out = torch.full((k, image.shape[0]) + tuple(patch), -77.0, device=DEV)          # junk: every element must be written
    di = image.to(DEV).contiguous()
    check(lib().hdf_sw_gather(ptr(di), image.shape[0], *image.shape[1:], *origin, *ext, *patch, mask, ptr(out), st()),
          "hdf_sw_gather")
    return out.cpu()


def test_gather_writes_every_element_for_every_mask():
    gen = torch.Generator().manual_seed(31)
    image = torch.randn((2, 11, 13, 9), generator=gen)
    for mask in range(8):
        got = _gather(image, (2, 3, 1), (7, 9, 5), (8, 12, 8), mask)
        assert torch.equal(got, sw_ref.gather_ref(image, (2, 3, 1), (7, 9, 5), (8, 12, 8), mask)), mask
        got = _gather(image, (2, 3, 1), (7, 9, 5), (8, 12, 7), mask)              # a row length the 4-wide form cannot take
        assert torch.equal(got, sw_ref.gather_ref(image, (2, 3, 1), (7, 9, 5), (8, 12, 7), mask)), mask
    # past one trip of the grid: 4096 x 256 threads, four elements each where the row length is a multiple of four
    big = torch.randn((2, 70, 70, 72), generator=gen)
    for patch, trip in (((64, 64, 68), 4 * 4096 * 256), ((40, 44, 50), 4096 * 256)):
        ext = (37, 44, 45)
        got = _gather(big, (5, 3, 2), ext, patch, 7)
        assert got.numel() > trip
        assert torch.equal(got, sw_ref.gather_ref(big, (5, 3, 2), ext, patch, 7))


def _device_tables(tables):
    """(tables on the device, floor on the device) through hdf_sw_importance_floor"""
    tab = torch.from_numpy(np.concatenate(tables)).to(DEV)
    floor = torch.full((1,), -5.0, device=DEV)
    check(lib().hdf_sw_importance_floor(ptr(tab), *[len(t) for t in tables], ptr(floor), st()), "hdf_sw_importance_floor")
    return tab, floor


def test_weights_and_floor_are_the_reference_map_bit_for_bit():
    for extent in sw_ref.EXTENTS:
        for s in sw_ref.SIGMA_SCALES:
            tables = sw_ref.tables_of(extent, s)
            tab, floor = _device_tables(tables)
            want_floor = sw_ref.floor_of(sw_ref.raw_weights(tables))
            assert floor.cpu().numpy().view(np.uint32)[0] == np.float32(want_floor).view(np.uint32), (extent, s)
            logits = torch.zeros((1, 1) + extent, device=DEV)
            psum, wsum = torch.zeros((1,) + extent, device=DEV), torch.zeros(extent, device=DEV)
            check(lib().hdf_sw_accumulate_tta(F32, ptr(logits), 0, 1, *extent, *extent, ptr(tab), ptr(floor), ptr(psum),
                                              ptr(wsum), *extent, 0, 0, 0, st()), "hdf_sw_accumulate_tta")
            sw_ref.check_weights(psum, wsum, extent, s)


@functools.lru_cache(maxsize=1)
def _plain_logits(c=3):
    return [mr.sw_logits(k, c) for k in range(len(mr.SW_WINDOWS))]


@pytest.mark.parametrize("dtype", ALL, ids=NAME.get)
def test_without_mirroring_and_weights_it_is_the_existing_entry(dtype):
    c = 3
    d, h, w = mr.SW_VOLUME
    acc = [[torch.zeros((c, d, h, w), device=DEV), torch.zeros((d, h, w), device=DEV)] for _ in range(2)]
    for ((z, y, x), (pd, ph, pw)), lg in zip(mr.SW_WINDOWS, _plain_logits()):
        dl = lg.to(DEV).to(TDT[dtype]).contiguous()
        check(lib().hdf_sw_accumulate(dtype, ptr(dl), c, pd, ph, pw, ptr(acc[0][0]), ptr(acc[0][1]), d, h, w, z, y, x, st()),
              "hdf_sw_accumulate")
        check(lib().hdf_sw_accumulate_tta(dtype, ptr(dl), 0, c, pd, ph, pw, pd, ph, pw, None, None, ptr(acc[1][0]),
                                          ptr(acc[1][1]), d, h, w, z, y, x, st()), "hdf_sw_accumulate_tta")
    assert torch.equal(acc[0][1], acc[1][1]) and float(acc[0][1].max()) == 5.0
    assert torch.equal(acc[0][0].view(torch.int32), acc[1][0].view(torch.int32))


def _run(dtype, windows, logits, mask, tables_of_window, acc, volume, patch):
    """hdf_sw_accumulate_tta window after window into acc = (prob_sum, weight_sum) on the device"""
    dev = {}
    for (origin, ext), lg in zip(windows, logits):
        tables = tables_of_window(ext)
        if tables is not None and ext not in dev:
            dev[ext] = _device_tables(tables)
        tab, floor = dev.get(ext, (None, None))
        dl = lg.to(DEV).to(TDT[dtype]).contiguous()
        check(lib().hdf_sw_accumulate_tta(dtype, ptr(dl), mask, lg.shape[1], *ext, *patch, ptr(tab), ptr(floor),
                                          ptr(acc[0]), ptr(acc[1]), *volume, *origin, st()), "hdf_sw_accumulate_tta")
    return acc[0].cpu(), acc[1].cpu()


def _reference(windows, logits, mask, tables_of_window, dt, volume, init):
    """accumulate_ref window by window (a clipped window has tables of its own)"""
    acc = init
    for win, lg in zip(windows, logits):
        acc = sw_ref.accumulate_ref([win], [lg], mask, tables_of_window(win[1]), dt, volume, acc)
    return acc


@pytest.mark.parametrize("dtype", ALL, ids=NAME.get)
def test_accumulation_past_the_cap(dtype):
    """ROUNDING sw_accumulate_tta.psum (MI355X, pytest -s): f32 0.226, bf16 0.226, f16 0.224 of the bound."""
    c, mask, patch = 3, 0b101, mr.SW_WINDOWS[0][1]
    gen = torch.Generator().manual_seed(640)
    logits = [rnd(torch.randn((4, c) + patch, generator=gen) * 2.0, dtype) for _ in mr.SW_WINDOWS]
    tables = functools.lru_cache(maxsize=None)(lambda ext: sw_ref.tables_of(ext, 1 / 8))
    init = (torch.zeros((c,) + mr.SW_VOLUME), torch.zeros(mr.SW_VOLUME))
    ref64 = _reference(mr.SW_WINDOWS, logits, mask, tables, torch.float64, mr.SW_VOLUME, init)
    ref32 = _reference(mr.SW_WINDOWS, logits, mask, tables, torch.float32, mr.SW_VOLUME, init)
    assert bool((ref64[1] == 0).any()) and mr.SW_WINDOWS[-1][1] != patch          # an uncovered region, a clipped window
    got = _run(dtype, mr.SW_WINDOWS, logits, mask, tables, [t.to(DEV) for t in init], mr.SW_VOLUME, patch)
    worst = sw_ref.check_accumulators(got, ref32, ref64, init, True, "past the cap")
    print("ROUNDING sw_accumulate_tta.psum %s %.3f" % (NAME[dtype], worst), flush=True)


SMALL_VOLUME = (11, 13, 9)
SMALL = [((7, 9, 5), (8, 12, 8), [(0, 0, 0), (4, 4, 4), (2, 3, 1)]),               # (0, 12, 8) is never reached
         ((1, 8, 8), (8, 8, 8), [(0, 0, 0), (3, 5, 1), (10, 2, 0)])]


@pytest.mark.parametrize("dtype", ALL, ids=NAME.get)
def test_small_windows_every_mask_weighted_or_not(dtype):
    gen = torch.Generator().manual_seed(77)
    worst = 0.0
    for ext, patch, origins in SMALL:
        windows = [(o, ext) for o in origins]
        for c in (2, 8):
            init = (torch.rand((c,) + SMALL_VOLUME, generator=gen), torch.randint(0, 3, SMALL_VOLUME, generator=gen).float())
            for mask in range(8):
                k = len(sw_ref.variants(mask))
                logits = [rnd(torch.randn((k, c) + patch, generator=gen) * 2.0, dtype) for _ in windows]
                for weighted in (False, True):
                    tables = (lambda e: sw_ref.tables_of(e, 1 / 8)) if weighted else (lambda e: None)
                    ref64 = _reference(windows, logits, mask, tables, torch.float64, SMALL_VOLUME, init)
                    ref32 = _reference(windows, logits, mask, tables, torch.float32, SMALL_VOLUME, init)
                    assert bool((ref64[1] == init[1].double()).any())
                    got = _run(dtype, windows, logits, mask, tables, [t.to(DEV) for t in init], SMALL_VOLUME, patch)
                    worst = max(worst, sw_ref.check_accumulators(got, ref32, ref64, init, weighted,
                                                                 "%s classes %d mask %d weighted %d" % (ext, c, mask, weighted)))
    print("ROUNDING sw_accumulate_tta.small %s %.3f" % (NAME[dtype], worst), flush=True)


def test_bad_arguments_are_refused_before_anything_is_launched():
    ext = (4, 4, 4)
    logits = torch.zeros((1, 2) + ext, device=DEV)
    psum, wsum = torch.full((2,) + ext, 3.0, device=DEV), torch.full(ext, 2.0, device=DEV)
    tab, floor = _device_tables(sw_ref.tables_of(ext, 1 / 8))
    image, out = torch.zeros((1,) + ext, device=DEV), torch.full((1, 1) + ext, 9.0, device=DEV)

    def accumulate(mask=0, tables=None, fl=None, origin=(0, 0, 0)):
        return lib().hdf_sw_accumulate_tta(F32, ptr(logits), mask, 2, *ext, *ext, ptr(tables), ptr(fl), ptr(psum), ptr(wsum),
                                           *ext, *origin, st())

    assert accumulate(mask=8) == HDF_ERR_ARG and b"mirror_mask" in lib().hdf_last_error()
    assert accumulate(tables=tab) == HDF_ERR_ARG and b"go together" in lib().hdf_last_error()
    assert accumulate(fl=floor) == HDF_ERR_ARG
    assert accumulate(origin=(0, 1, 0)) == HDF_ERR_ARG and b"outside" in lib().hdf_last_error()
    assert lib().hdf_sw_gather(ptr(image), 1, *ext, 0, 0, 0, *ext, *ext, 8, ptr(out), st()) == HDF_ERR_ARG
    assert lib().hdf_sw_gather(ptr(image), 1, *ext, 1, 0, 0, *ext, *ext, 0, ptr(out), st()) == HDF_ERR_ARG
    assert lib().hdf_sw_gather(ptr(image), 1, *ext, 0, 0, 0, *ext, 4, 3, 4, 0, ptr(out), st()) == HDF_ERR_ARG    # e > P
    torch.cuda.synchronize()
    assert float(psum.min()) == float(psum.max()) == 3.0 and float(wsum.min()) == float(wsum.max()) == 2.0
    assert float(out.min()) == float(out.max()) == 9.0
    assert accumulate(tables=tab, fl=floor) == 0                                     # and the good call goes through


def _leading_means(psum64, wsum64):
    """(first argmax of prob_sum / weight_sum in fp64, excluded: the two leading means differ by less than 4 fp32 ulp) --
    metrics_ref.finalize_reference for a weight sum that may be below 1"""
    mean = psum64 / wsum64
    top2 = mean.topk(2, 0).values
    gap = top2[0] - top2[1]
    ulp = torch.exp2(torch.floor(torch.log2(top2[0].clamp_min(1e-300))) - 23)
    return mr.first_argmax(mean, 0), (gap > 0) & (gap < 4 * ulp)


def test_predict_with_gaussian_importance_and_mirroring_end_to_end():
    """ROUNDING sw_predict_tta.psum (MI355X, pytest -s): 0.229 of the bound on the 48x40x32 image (weight_sum 0.227),
    0.218 (0.197) on the clipped 20x40x32 one; no label differed outside the excluded voxels."""
    from hdf_rt import inference
    from models.HDenseFormer import HDenseFormer
    from oracle import detgen
    from oracle import hdf_oracle as orc
    g = np.load(os.path.join(GOLDEN, "g8_sliding_window.npz"), allow_pickle=False)
    in_ch, n_cls, nf, td = [int(v) for v in g["cfg"]]
    patch = tuple(int(v) for v in g["patch"])
    step = tuple(int(v) for v in g["step"])
    size = tuple(int(v) for v in g["image_size"])
    net = HDenseFormer(in_ch, n_cls, nf, image_size=patch, transformer_depth=td)
    net.load_state_dict(orc.det_model(in_ch, n_cls, nf, patch, td))
    net = net.cuda().eval()
    net.compute_dtype = "fp32"
    full = torch.from_numpy(detgen.det_input(1, in_ch, size, tag="sw")[0])
    before = inference.sliding_window_predict(net, full, patch, step, return_probabilities=True)
    opts = dict(importance="gaussian", mirror_axes=(0, 2))
    for image in (full, full[:, :20]):
        lab, mean = inference.sliding_window_predict(net, image, patch, step, return_probabilities=True, **opts)
        psum, wsum = inference._sliding_window_sums(net, image, patch, step, 4, "gaussian", 1 / 8, (0, 2))
        assert torch.equal(mean, psum / wsum) and tuple(lab.shape) == tuple(image.shape[1:])
        answers = []

        def device_net(batch):
            with torch.no_grad():
                answers.append(net(batch.to(DEV))[0].float().cpu())
            return answers[-1]

        _, _, p64, w64 = sw_ref.predict_ref(device_net, image, patch, step, dt=torch.float64, **opts)
        replay = iter(answers)                                                        # the same answers, accumulated in fp32
        _, _, p32, w32 = sw_ref.predict_ref(lambda batch: next(replay), image, patch, step, dt=torch.float32, **opts)
        assert len(answers) > 1 and answers[0].shape[0] == 4                          # one window's four variants a forward
        worst_w = check_fp32_sum(wsum.cpu(), w64, 4 * float((w32.double() - w64).abs().max()), "weight_sum")
        worst_p = check_fp32_sum(psum.cpu(), p64, 4 * float((p32.double() - p64).abs().max()), "prob_sum")
        print("ROUNDING sw_predict_tta.psum %s %.3f wsum %.3f" % (tuple(image.shape[1:]), worst_p, worst_w), flush=True)
        want, excluded = _leading_means(p64, w64)
        assert float(excluded.double().mean()) <= 1e-3
        got = lab.cpu().long()
        assert torch.equal(got[~excluded], want[~excluded]), int((got != want)[~excluded].sum())
    after = inference.sliding_window_predict(net, full, patch, step, return_probabilities=True)
    assert torch.equal(before[0], after[0]) and torch.equal(before[1].view(torch.int32), after[1].view(torch.int32))
