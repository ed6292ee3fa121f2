"""What the per-region order statistics cost on the device against np.quantile per id on the host.  One process, the 128^3
volume of 36 truth lesions of tools/lesion_hd_bench.py labelled on the device and the C = 2 image channels of
tools/measure_bench.py (a uniform one and a signed one with exponents over 2^-20 .. 2^20).

  region_quantiles   hdf_rt.region_quantiles(ids, image, (0.1, 0.5, 0.9)): one hdf_cc_quantiles call, nothing copied
  region_measure     hdf_rt.region_measure on the same inputs: the yardstick -- both pay for the walk that leaves the boxes;
                     the select reads the boxes four times per channel, the measurement twice
  np.quantile        on the host, the id map and the image already there (no copy is timed): per id and channel, the three
                     levels in one call, on one thread
  one id, 128^3      one id that fills the volume: what one workgroup per (id, channel) costs at its worst

The device's outputs are compared with tests/quantile_ref.py first, every byte.  Device times are HIP events around the
call after warm-up, the median of --reps.  Prints one JSON line.

    python tools/quantile_bench.py [--size 128] [--reps 20] [--seed 0] [--capacity 4096]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "h-denseformer_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
import numpy as np
import torch
from scipy import ndimage as ndi

import quantile_ref as qr
from hdf_rt import connected_components, region_measure, region_quantiles
from lesion_hd_bench import gpu_ms, volume

DEV = torch.device("cuda", 0)
LEVELS = (0.1, 0.5, 0.9)


def _compare(ids, img, ids_h, image, capacity, what):
    count, values, res = region_quantiles(ids, img, LEVELS, capacity)
    got = dict(count=count.cpu().numpy(), values=values.cpu().numpy(), result=res.cpu().tolist())
    want = qr.quantiles(ids_h, image, LEVELS, capacity)
    bad = qr.mismatches(got, want)
    if bad:
        raise SystemExit(f"the device and the restatement disagree ({what}): {bad}")
    return want


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--capacity", type=int, default=4096)
    a = ap.parse_args()
    shape = (a.size,) * 3
    _, truth = volume(a.size, a.seed)
    rng = np.random.default_rng(a.seed + 1)
    image = np.stack([rng.random(shape, dtype=np.float32),
                      (rng.uniform(1.0, 2.0, shape) * np.exp2(rng.integers(-20, 21, shape)) * rng.choice([-1.0, 1.0], shape))
                      .astype(np.float32)])
    ids, count = connected_components(torch.from_numpy(truth).to(DEV), 26, 0)
    img = torch.from_numpy(image).to(DEV)
    n = int(count)
    ids_h = ids.cpu().numpy()
    want = _compare(ids, img, ids_h, image, a.capacity, "lesions")
    row = dict(volume=list(shape), channels=2, levels=list(LEVELS), lesions=n, capacity=a.capacity, reps=a.reps,
               lesion_voxels=int(want["result"][1]))
    objects = ndi.find_objects(ids_h)
    row["box_voxels"] = sum(int(np.prod([s.stop - s.start for s in sl])) for sl in objects)
    row["region_quantiles_ms"] = gpu_ms(lambda: region_quantiles(ids, img, LEVELS, a.capacity), a.reps)
    row["region_measure_ms"] = gpu_ms(lambda: region_measure(ids, img, a.capacity), a.reps)
    t0 = time.perf_counter()
    for c in range(2):
        for i, sl in enumerate(objects, 1):                      # (the box first: what a careful host loop does)
            np.quantile(image[c][sl][ids_h[sl] == i].astype(np.float64), LEVELS)
    row["np_quantile_per_id_ms"] = (time.perf_counter() - t0) * 1e3
    one = torch.ones(shape, dtype=torch.int32, device=DEV)
    _compare(one, img, np.ones(shape, np.int32), image, 1, "one id")
    row["one_id_full_volume_ms"] = gpu_ms(lambda: region_quantiles(one, img, LEVELS, 1), a.reps)
    print(json.dumps(row))


if __name__ == "__main__":
    main()
