"""What the region measurements cost on the device against the scipy calls they replace.  One process, the 128^3 volume of
36 truth lesions of tools/lesion_hd_bench.py (seeded ellipsoids on a jittered grid) labelled on the device, and C = 2
image channels (a uniform one and a signed one with exponents over 2^-20 .. 2^20).

  region_measure   hdf_rt.region_measure(ids, image): one hdf_cc_measure call, nothing copied
  component table  hdf_rt.component_table(volume, ids) on the same ids: the yardstick -- both read the id map once; the
                   measurement's first pass additionally reads C fp32 channels where an id counts, and its two slab passes
                   read the boxes of the ids
  scipy            on the host, the id map and the image already there (no copy is timed): sum_labels, mean, variance,
                   minimum, maximum, minimum_position, maximum_position, center_of_mass, per channel, one run

The device's outputs are compared with tests/measure_ref.py first (integers, extrema and positions exactly, the fp64 sums
to its derived bounds).  Device times are HIP events around the call after warm-up, the median of --reps.  Prints one JSON
line.

    python tools/measure_bench.py [--size 128] [--reps 20] [--seed 0] [--capacity 4096]"""
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

import measure_ref as mr
from hdf_rt import component_table, connected_components, region_measure
from lesion_hd_bench import gpu_ms, volume

DEV = torch.device("cuda", 0)


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
    vol = torch.from_numpy(truth).to(DEV)
    ids, count = connected_components(vol, 26, 0)
    img = torch.from_numpy(image).to(DEV)
    n = int(count)

    geom, stats, pos, res = region_measure(ids, img, a.capacity)
    ids_h = ids.cpu().numpy()
    got = dict(geom=geom.cpu().numpy(), stats=stats.cpu().numpy(), pos=pos.cpu().numpy(), result=res.cpu().tolist())
    want = mr.measure(ids_h, image, a.capacity)
    bad = mr.mismatches(got, want)
    if bad:
        raise SystemExit(f"the device and the restatement disagree: {bad}")
    row = dict(volume=list(shape), channels=2, lesions=n, capacity=a.capacity, reps=a.reps,
               lesion_voxels=int(want["result"][1]), worst_error_over_bound=mr.worst(got, want))
    box = 0
    for sl in ndi.find_objects(ids_h):
        box += int(np.prod([s.stop - s.start for s in sl]))
    row["box_voxels"] = box
    row["region_measure_ms"] = gpu_ms(lambda: region_measure(ids, img, a.capacity), a.reps)
    row["component_table_ms"] = gpu_ms(lambda: component_table(vol, ids, capacity=a.capacity), a.reps)
    index = np.arange(1, n + 1)
    t0 = time.perf_counter()
    for c in range(2):
        x = image[c]
        for fn in (ndi.sum_labels, ndi.mean, ndi.variance, ndi.minimum, ndi.maximum, ndi.minimum_position,
                   ndi.maximum_position, ndi.center_of_mass):
            fn(x, ids_h, index)
    row["scipy_eight_calls_ms"] = (time.perf_counter() - t0) * 1e3
    print(json.dumps(row))


if __name__ == "__main__":
    main()
