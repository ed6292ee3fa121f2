"""The tail of ONE sliding-window window with a Gaussian importance map and mirror test-time augmentation, timed on one
MI355X (HIP-event medians, everything resident on the device): hdf_sw_gather + hdf_sw_accumulate_tta for K = 1, 4, 8
variants, weighted or not, next to hdf_sw_accumulate (the plain tail) and to the torch composition they replace -- flip
copies of the input, per variant a softmax, a flip back and two indexed read-modify-writes under a 3-D weight map.

  python tools/sw_tta_bench.py                  one JSON object per line (DESIGN.md 6b quotes them)
  HDF_LIB_PATH=<an older libhdf_hip.so> python tools/sw_tta_bench.py --plain-only      hdf_sw_accumulate of that build
"""
import json
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "h-denseformer_amd")):
    sys.path.insert(0, p)
import numpy as np
import torch

from hdf_rt import _lib
from hdf_rt._lib import check, lib, ptr, stream_ptr
from hdf_rt.inference import gaussian_tables

DEV = torch.device("cuda", 0)
P, VOL, ORIGIN, CH, N_CLS = (128, 128, 128), (160, 160, 160), (16, 16, 16), 4, 2
MASKS = {1: 0, 4: 0b101, 8: 0b111}
AXES = {0: (), 0b101: (0, 2), 0b111: (0, 1, 2)}


def gpu_ms(fn, inner=10, reps=9, warm=2):
    """median over reps of the time of `inner` back-to-back calls, per call"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / inner)
    return sorted(ts)[len(ts) // 2]


def emit(**kw):
    print(json.dumps(kw), flush=True)


def main(plain_only):
    gen = torch.Generator().manual_seed(5)
    psum, wsum = torch.zeros((N_CLS,) + VOL, device=DEV), torch.zeros(VOL, device=DEV)
    logits8 = (torch.randn((8, N_CLS) + P, generator=gen) * 2.0).to(DEV).bfloat16()
    plain = lambda: check(lib().hdf_sw_accumulate(_lib.BF16, ptr(logits8), N_CLS, *P, ptr(psum), ptr(wsum), *VOL, *ORIGIN,
                                                  stream_ptr()), "hdf_sw_accumulate")
    emit(row="hdf_sw_accumulate", lib=os.path.basename(_lib.LIB_PATH), ms=round(gpu_ms(plain), 4))
    if plain_only:
        return
    image = torch.randn((CH,) + VOL, generator=gen).to(DEV)
    tables = gaussian_tables(P)
    tab = torch.from_numpy(np.concatenate(tables)).to(DEV)
    floor = torch.empty(1, device=DEV)
    check(lib().hdf_sw_importance_floor(ptr(tab), *P, ptr(floor), stream_ptr()), "hdf_sw_importance_floor")
    tz, ty, tx = (torch.from_numpy(t).to(DEV) for t in tables)
    wmap = ((tz[:, None, None] * ty[None, :, None]) * tx[None, None, :] / (tz[64] * ty[64] * tx[64])).float()
    z, y, x = ORIGIN
    win = (slice(z, z + P[0]), slice(y, y + P[1]), slice(x, x + P[2]))
    for K, mask in MASKS.items():
        data = torch.empty((K, CH) + P, device=DEV)
        logits = logits8[:K].contiguous()
        gather = lambda: check(lib().hdf_sw_gather(ptr(image), CH, *VOL, *ORIGIN, *P, *P, mask, ptr(data), stream_ptr()),
                               "hdf_sw_gather")
        subsets = [[a for a in AXES[mask] if m >> a & 1] for m in range(8) if m & ~mask == 0]

        def torch_gather():
            src = image[(slice(None),) + win]
            return torch.stack([torch.flip(src, [1 + a for a in s]) if s else src for s in subsets])

        emit(row="gather", K=K, hip_ms=round(gpu_ms(gather), 4), torch_ms=round(gpu_ms(torch_gather), 4))
        for weighted in (False, True):
            t, f = (tab, floor) if weighted else (None, None)
            tail = lambda: check(lib().hdf_sw_accumulate_tta(_lib.BF16, ptr(logits), mask, N_CLS, *P, *P, ptr(t), ptr(f),
                                                             ptr(psum), ptr(wsum), *VOL, *ORIGIN, stream_ptr()),
                                 "hdf_sw_accumulate_tta")

            def torch_tail():
                for k, s in enumerate(subsets):
                    p = torch.softmax(logits[k].float(), 0)
                    if s:
                        p = torch.flip(p, [1 + a for a in s])
                    if weighted:
                        psum[(slice(None),) + win] += p * wmap * (1.0 / K)
                        wsum[win] += wmap * (1.0 / K)
                    else:
                        psum[(slice(None),) + win] += p * (1.0 / K)
                        wsum[win] += 1.0 / K

            emit(row="accumulate", K=K, weighted=weighted, hip_ms=round(gpu_ms(tail), 4),
                 torch_ms=round(gpu_ms(torch_tail), 4))


if __name__ == "__main__":
    main("--plain-only" in sys.argv[1:])
