"""The metric, staging and inference-tail C entries of include/hdf.h called directly, past the grid caps of their kernels
(csrc/metrics.hip, csrc/augment.hip), where a wrong grid stride, an uncovered tail or a lost count would show -- the existing tests go through
the Python wrappers at 8^3 .. 12x20x24 voxels, inside one trip of every grid-stride loop:
  hdf_dice_counts, hdf_confusion_matrix (1024 x 256)   V = 63*65*67 = 274 365, N = 3, C = 5: exact integers against a CPU
      count of first-maximum argmaxes of the storage-rounded logits (16-bit logits x 0.25: exact ties are common);
      V in {1, 255, 257} x C in {2, 8}; accumulate = 1 twice = 2 x, accumulate = 0 overwrites
  hdf_confusion_matrix_labels (1024 x 256)             n = 274 365, about 1 % labels >= C on either side, dropped
  hdf_sw_accumulate (4096 x 256)                       window 96x104x112 = 1 118 208 voxels in a 100x110x120 volume, four
      overlapping origins, one clipped window, a region no window covers; cnt exact, psum per element within
      4 |torch fp32 accumulation - fp64| + 2^-24 |ref| (hip_util.check_fp32_sum)
  hdf_sw_finalize (8192 x 256)                         V = 2 097 152 + 777 crafted psum / cnt: 0 where cnt == 0, the first
      class on an exact tie, else the fp64 argmax of psum / cnt except where the two leading means differ by less than
      4 fp32 ulp (<= 0.1 % of the voxels, a condition on the inputs that tests/test_loss_check_cpu.py checks)
  hdf_onehot_from_labels (4096 x 256)                  V = 1 048 576 + 333, N = 2, C = 3; C = 9 with labels up to 255
  hdf_normalize_mr / _petct (512 x 256, 4096 x 256)    V = 104*101*103 = 1 081 912; MR bit-exact (an all-zero channel, an
      all-negative one, the maximum at the last voxel / at voxel 0); PET/CT channel 0 and the untouched channel 2
      bit-exact, channel 1 within the spread of its fp32 restatement when mean and std each move one fp32 ulp
Out of scope: NaN / Inf logits in the metric kernels -- torch.argmax treats NaN as the maximum, a strict `>` never selects
it: they differ there by design.
Worst error / bound printed on an MI355X ("ROUNDING ...", pytest -s): sw_accumulate.psum f32 0.226, bf16 0.228, f16 0.227;
petct.channel1 0.000 (zscore and constant); every other check in here is exact."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import metrics_ref as mr  # noqa: E402
from hdf_rt._lib import BF16, F16, F32, check, lib, ptr  # noqa: E402
from hip_util import DEV, TDT, check_fp32_sum, rnd, st  # noqa: E402
from oracle import sw_oracle  # noqa: E402

NAME = {F32: "f32", BF16: "bf16", F16: "f16"}
ALL = [F32, BF16, F16]
BIG_V = 63 * 65 * 67


def _onehot(lab, c):
    return torch.nn.functional.one_hot(lab, c).movedim(-1, 1).float().contiguous()


def _dice_counts(dtype, lg, tg):
    n, c, v = lg.shape
    out = torch.full((n, 8, 3), -7, dtype=torch.int64, device=DEV)
    check(lib().hdf_dice_counts(dtype, ptr(lg), ptr(tg), n, c, v, ptr(out), st()), "hdf_dice_counts")
    return out.cpu()


def _confusion(dtype, lg, tg, conf, accumulate):
    n, c, v = lg.shape
    check(lib().hdf_confusion_matrix(dtype, ptr(lg), ptr(tg), n, c, v, ptr(conf), accumulate, st()), "hdf_confusion_matrix")
    return conf.cpu()


def _metric_case(dtype, n, c, v, seed):
    logits, lab = mr.metric_inputs(n, c, v, seed, 1.0 if dtype == F32 else 0.25)
    r = rnd(logits, dtype)
    pred = mr.first_argmax(r)
    return r.to(DEV).to(TDT[dtype]), _onehot(lab, c).to(DEV), lab, pred


@pytest.mark.parametrize("dtype", ALL, ids=NAME.get)
@pytest.mark.parametrize("n,c,v", [(3, 5, BIG_V), (1, 2, 1), (1, 8, 1), (1, 2, 255), (1, 8, 255), (1, 2, 257), (1, 8, 257)])
def test_dice_counts_and_confusion_matrix_are_exact(n, c, v, dtype):
    lg, tg, lab, pred = _metric_case(dtype, n, c, v, 40 + c)
    if v == BIG_V and dtype != F32:
        top2 = lg.float().topk(2, 1).values
        assert int((top2[:, 0] == top2[:, 1]).sum()) > 100          # the tie rule is exercised
    want = mr.confusion_of(lab, pred, c)
    conf = torch.full((8, 8), 12345, dtype=torch.int64, device=DEV)
    got = _confusion(dtype, lg, tg, conf, 0)                         # accumulate = 0 overwrites what was there
    assert torch.equal(got, want), (got, want)
    counts = _dice_counts(dtype, lg, tg)
    assert torch.equal(counts[:, :c], mr.dice_counts_of(lab, pred, c)[:, :c])
    # the two entries agree with each other, sample by sample
    total = torch.zeros(8, 8, dtype=torch.int64)
    for k in range(n):
        one = _confusion(dtype, lg[k:k + 1].contiguous(), tg[k:k + 1].contiguous(), conf, 0)
        assert torch.equal(counts[k, :c, 0], one.diagonal()[:c])
        assert torch.equal(counts[k, :c, 1], one.sum(0)[:c]) and torch.equal(counts[k, :c, 2], one.sum(1)[:c])
        total += one
    assert torch.equal(total, want)
    # accumulate = 1 twice on a zeroed matrix: exactly twice the single call
    conf.zero_()
    _confusion(dtype, lg, tg, conf, 1)
    assert torch.equal(_confusion(dtype, lg, tg, conf, 1), 2 * want)


def test_confusion_matrix_of_label_maps_is_exact():
    c = 5
    tgt, pred = mr.label_maps(BIG_V, c, 60)
    assert int((tgt >= c).sum()) > 1000 and int((pred >= c).sum()) > 1000
    want = mr.confusion_of(tgt, pred, c)
    conf = torch.full((8, 8), 999, dtype=torch.int64, device=DEV)
    dt, dp = tgt.to(DEV), pred.to(DEV)
    check(lib().hdf_confusion_matrix_labels(ptr(dt), ptr(dp), c, BIG_V, ptr(conf), 0, st()), "labels")
    assert torch.equal(conf.cpu(), want)
    check(lib().hdf_confusion_matrix_labels(ptr(dt), ptr(dp), c, BIG_V, ptr(conf), 1, st()), "labels")
    assert torch.equal(conf.cpu(), 2 * want)
    for n in (1, 255, 257):
        check(lib().hdf_confusion_matrix_labels(ptr(dt), ptr(dp), c, n, ptr(conf), 0, st()), "labels")
        assert torch.equal(conf.cpu(), mr.confusion_of(tgt[:n], pred[:n], c))


@pytest.mark.parametrize("dtype", ALL, ids=NAME.get)
def test_sliding_window_accumulation_past_the_cap(dtype):
    c = 3
    d, h, w = mr.SW_VOLUME
    logits = [rnd(mr.sw_logits(k, c), dtype) for k in range(len(mr.SW_WINDOWS))]
    p64, c64 = mr.sw_reference(mr.SW_WINDOWS, logits, c, torch.float64)
    p32, _ = mr.sw_reference(mr.SW_WINDOWS, logits, c, torch.float32)
    assert bool((c64 == 0).any()) and float(c64.max()) == 5.0       # an uncovered region, and all five windows overlap
    psum = torch.zeros((c, d, h, w), dtype=torch.float32, device=DEV)
    cnt = torch.zeros((d, h, w), dtype=torch.float32, device=DEV)
    for ((z, y, x), (pd, ph, pw)), lg in zip(mr.SW_WINDOWS, logits):
        dl = lg.to(DEV).to(TDT[dtype]).contiguous()
        check(lib().hdf_sw_accumulate(dtype, ptr(dl), c, pd, ph, pw, ptr(psum), ptr(cnt), d, h, w, z, y, x, st()),
              "hdf_sw_accumulate")
    assert torch.equal(cnt.cpu().double(), c64)
    got = psum.cpu()
    assert bool((got[:, c64 == 0] == 0).all())
    worst = check_fp32_sum(got, p64, 4 * float((p32.double() - p64).abs().max()), "psum")
    print("ROUNDING sw_accumulate.psum %s %.3f" % (NAME[dtype], worst), flush=True)


@pytest.mark.parametrize("c", [2, 8])
def test_sliding_window_vote_past_the_cap(c):
    psum, cnt, tied = mr.finalize_inputs(c)
    want, excluded = mr.finalize_reference(psum, cnt)
    assert float(excluded.double().mean()) <= 1e-3
    label = torch.full((mr.FIN_V,), 77, dtype=torch.uint8, device=DEV)
    dp, dc = psum.to(DEV), cnt.to(DEV)
    check(lib().hdf_sw_finalize(ptr(dp), ptr(dc), c, mr.FIN_V, ptr(label), st()), "hdf_sw_finalize")
    got = label.cpu().long()
    assert bool((got[cnt == 0] == 0).all())
    assert torch.equal(got[~excluded], want[~excluded]), int((got != want)[~excluded].sum())
    both = tied & (cnt > 0)
    assert int(both.sum()) > 50000 and torch.equal(got[both], want[both])    # exact ties: the first class


def test_onehot_from_labels_past_the_cap():
    def run(lab, c):
        n, v = lab.shape
        oh = torch.full((n, c, v), -3.0, dtype=torch.float32, device=DEV)
        dl = lab.to(DEV)
        check(lib().hdf_onehot_from_labels(ptr(dl), ptr(oh), n, c, v, st()), "hdf_onehot_from_labels")
        assert torch.equal(oh.cpu(), mr.to_onehot_batch(lab, c))

    run(mr.onehot_labels(2, 1048576 + 333, 5), 3)        # labels 3 and 4 are "no other class": background
    run(mr.onehot_labels(1, 4099, 256), 9)               # more classes than the 8-slot kernels take, labels up to 255


def _normalize(entry, img, *args):
    c, v = img.shape
    d = img.to(DEV).contiguous()
    ws = torch.zeros(lib().hdf_normalize_workspace_bytes(c), dtype=torch.uint8, device=DEV)
    check(getattr(lib(), entry)(ptr(d), c, v, *args, ptr(ws), st()), entry)
    return d.cpu()


def test_mr_normalize_past_the_caps_is_bit_exact():
    img = mr.mr_image()
    assert float(img[0].abs().max()) == 0 and float(img[1].max()) < 0
    assert int(img[2].argmax()) == mr.NORM_V - 1 and int(img[3].argmax()) == 0
    got = _normalize("hdf_normalize_mr", img)
    want = torch.from_numpy(sw_oracle.mr_normalize(img.numpy()))
    assert torch.equal(got, want)
    assert float(got[2, -1]) == 1.0 and float(got[3, 0]) == 1.0 and float(got[1].min()) >= 1.0


@pytest.mark.parametrize("constant", [False, True], ids=["zscore", "constant"])
def test_petct_normalize_past_the_caps(constant):
    img = mr.petct_image(constant)
    got = _normalize("hdf_normalize_petct", img, 40.0, 400.0)
    want0 = torch.from_numpy(sw_oracle.pet_ct_normalize(img.numpy(), 40, 400)[0])
    assert torch.equal(got[0], want0) and float(got[0].min()) == -1.0 and float(got[0].max()) == 1.0
    assert torch.equal(got[2], img[2])
    ref, spread = mr.petct_channel1(img[1])
    err = (got[1].double() - ref.double()).abs()
    assert bool((err <= spread).all()), (float(err.max()), int((err > spread).sum()))
    if constant:
        assert float(got[1].abs().max()) == 0.0                      # (3.5 - 3.5) / (0 + 1e-3)
    else:
        assert float(spread.max()) < 1e-5 and abs(float(got[1].double().mean())) < 1e-5
    print("ROUNDING petct.channel1 %s %.3f" % ("constant" if constant else "zscore",
                                               float((err / spread.clamp_min(1e-300)).max())), flush=True)
