"""CPU side of tests/test_gpu_metrics_inference.py: seeded inputs past the grid caps of the metric, staging and
inference-tail kernels of csrc/metrics.hip and csrc/augment.hip, and plain counts / fp64 restatements to hold them to.  No GPU in here."""
import functools

import numpy as np
import torch

MAXC = 8


def first_argmax(x, dim=1):
    """index of the FIRST maximum along dim (torch.argmax's documented tie rule, which the kernels' strict `>` mirrors),
    spelled out so that no tie-breaking of a vectorised argmax enters the reference"""
    c = x.shape[dim]
    shape = [1] * x.dim()
    shape[dim] = c
    idx = torch.arange(c).view(shape).expand_as(x)
    mx = x.max(dim, keepdim=True).values
    return torch.where(x == mx, idx, torch.full_like(idx, c)).min(dim).values


def confusion_of(tgt, pred, c):
    """[8, 8] int64, rows = target class, columns = predicted class; labels >= c on either side are dropped"""
    tgt, pred = tgt.flatten().long(), pred.flatten().long()
    keep = (tgt < c) & (pred < c)
    return torch.bincount(tgt[keep] * MAXC + pred[keep], minlength=MAXC * MAXC).view(MAXC, MAXC)


def dice_counts_of(tgt, pred, c):
    """[N, 8, 3] int64: (|P = k and T = k|, |P = k|, |T = k|) per sample and class"""
    n = tgt.shape[0]
    out = torch.zeros(n, MAXC, 3, dtype=torch.int64)
    for k in range(c):
        pk, tk = (pred == k).flatten(1), (tgt == k).flatten(1)
        out[:, k, 0], out[:, k, 1], out[:, k, 2] = (pk & tk).sum(1), pk.sum(1), tk.sum(1)
    return out


def metric_inputs(n, c, v, seed, mul):
    """logits fp32 [n, c, v] (scaled by mul: 0.25 makes exact ties common once rounded to 16 bits), labels [n, v]"""
    gen = torch.Generator().manual_seed(seed)
    return torch.randn((n, c, v), generator=gen) * mul, torch.randint(0, c, (n, v), generator=gen)


def label_maps(n, c, seed):
    """two uint8 class maps with about 1 % labels >= c on either side"""
    gen = torch.Generator().manual_seed(seed)
    maps = []
    for _ in range(2):
        m = torch.randint(0, c, (n,), generator=gen)
        stray = torch.rand(n, generator=gen) < 0.01
        m[stray] = torch.randint(c, 256, (int(stray.sum()),), generator=gen)
        maps.append(m.to(torch.uint8))
    return maps


# ------------------------------------------------------------------------------------------------ sliding-window tail
SW_VOLUME = (100, 110, 120)
# (origin, window): four overlapping full windows -- (4, 6, 8) ends flush with the far corner, two mix the near and far
# origins -- and one clipped window; no window reaches e.g. (0, 109, 119)
SW_WINDOWS = [((0, 0, 0), (96, 104, 112)), ((4, 6, 8), (96, 104, 112)), ((0, 6, 0), (96, 104, 112)),
              ((4, 0, 8), (96, 104, 112)), ((60, 0, 0), (40, 104, 112))]


def sw_logits(k, c, seed=500):
    gen = torch.Generator().manual_seed(seed + k)
    return torch.randn((c,) + SW_WINDOWS[k][1], generator=gen) * 2.0


def sw_reference(windows, logits, c, dt):
    """psum [c, D, H, W] and cnt [D, H, W] of the oracle's accumulation (oracle/sw_oracle.py sliding_window: softmax per
    window, sum and count per voxel) in dtype dt"""
    psum = torch.zeros((c,) + SW_VOLUME, dtype=dt)
    cnt = torch.zeros(SW_VOLUME, dtype=dt)
    for ((z, y, x), (d, h, w)), lg in zip(windows, logits):
        psum[:, z:z + d, y:y + h, x:x + w] += torch.softmax(lg.to(dt), 0)
        cnt[z:z + d, y:y + h, x:x + w] += 1
    return psum, cnt


FIN_V = 2097152 + 777


@functools.lru_cache(maxsize=2)
def finalize_inputs(c, seed=700):
    """crafted (psum fp32 [c, V], cnt fp32 [V], tied [V] bool): counts 0..4 (about a fifth 0, with junk left in psum there),
    means from a softmax, and on about 5 % of the voxels the two leading classes tied exactly at the top"""
    gen = torch.Generator().manual_seed(seed + c)
    cnt = torch.randint(0, 5, (FIN_V,), generator=gen).float()
    psum = torch.softmax(torch.randn((c, FIN_V), generator=gen) * 2.0, 0) * cnt.clamp_min(1.0)
    tied = torch.rand(FIN_V, generator=gen) < 0.05
    a = torch.randint(0, c - 1, (FIN_V,), generator=gen)
    b = a + 1 + torch.randint(0, 1 << 20, (FIN_V,), generator=gen) % (c - 1 - a)
    top = psum.max(0).values * 1.25
    col = torch.arange(FIN_V)
    pa, pb = psum[a, col], psum[b, col]
    psum[a, col] = torch.where(tied, top, pa)
    psum[b, col] = torch.where(tied, top, pb)
    return psum.contiguous(), cnt, tied


def finalize_reference(psum, cnt):
    """(label int64 [V], excluded bool [V]): fp64 first argmax of psum / cnt, 0 where cnt == 0; excluded where the two
    leading means differ, but by less than 4 fp32 ulp of the larger (an fp32 division may order them either way)"""
    covered = cnt > 0
    mean = psum.double() / cnt.double().clamp_min(1.0)
    label = torch.where(covered, first_argmax(mean, 0), torch.zeros(cnt.shape, dtype=torch.int64))
    top2 = mean.topk(2, 0).values
    gap = top2[0] - top2[1]
    ulp = torch.exp2(torch.floor(torch.log2(top2[0].clamp_min(1e-300))) - 23)
    return label, covered & (gap > 0) & (gap < 4 * ulp)


# ------------------------------------------------------------------------------------------------ normalisation
NORM_V = 104 * 101 * 103


def mr_image(seed=900):
    """[4, V] fp32: channel 0 all zero, 1 all negative, 2 with its maximum at the very last voxel, 3 at voxel 0"""
    gen = torch.Generator().manual_seed(seed)
    img = torch.randn((4, NORM_V), generator=gen)
    img[0] = 0.0
    img[1] = -img[1].abs() - 0.125
    img[2, -1] = img[2].max() + 3.0
    img[3, 0] = img[3].max() + 2.0
    return img


def petct_image(constant, seed=901):
    """[3, V] fp32: CT-like channel 0 (clipped at 40 +- 400), channel 1 to be z-scored (constant 3.5: std 0, the divisor
    is the 1e-3 alone), channel 2 untouched"""
    gen = torch.Generator().manual_seed(seed)
    img = torch.randn((3, NORM_V), generator=gen)
    img[0] = img[0] * 300.0 + 40.0
    img[1] = 3.5 if constant else img[1] * 50.0 + 100.0
    return img


def petct_channel1(x):
    """(reference fp32 [V], allowance fp64 [V]): mean and population std of the fp32 channel in fp64, both rounded to fp32,
    then the kernel's fp32 operations in its order, (x - mean) / (std + 1e-3f).  The allowance is the spread of that when
    mean and std each move one fp32 ulp either way: a device summation order may land on the other side of one rounding."""
    xd = x.double()
    mean = xd.mean()
    sd = ((xd - mean) ** 2).mean().sqrt()
    m32, s32 = mean.float(), sd.float()
    eps = torch.tensor(1e-3, dtype=torch.float32)

    def apply(m, s):
        return (x - m) / (s + eps)

    ref = apply(m32, s32)
    inf = torch.tensor(float("inf"))
    spread = torch.zeros_like(xd)
    for m in (torch.nextafter(m32, -inf), m32, torch.nextafter(m32, inf)):
        for s in (torch.nextafter(s32, -inf).clamp_min(0.0), s32, torch.nextafter(s32, inf)):
            spread = torch.maximum(spread, (apply(m, s).double() - ref.double()).abs())
    return ref, spread


def onehot_labels(n, v, hi, seed=950):
    return torch.randint(0, hi, (n, v), generator=torch.Generator().manual_seed(seed)).to(torch.uint8)


def to_onehot_batch(lab, c):
    from oracle import sw_oracle
    return torch.from_numpy(np.stack([sw_oracle.to_onehot(m.numpy(), c) for m in lab]))
