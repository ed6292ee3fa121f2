"""Device time per class of hdf_surface_distances (mask flags, two exact squared distance transforms, gather, select) on
the volumes a user scores -- 144^3 and 240x240x155 -- with seeded three-label maps resident on the device, HIP events
around each call after a warm-up; beside it the host time of the scipy restatement of the same definitions
(tests/surface_ref.py) on the same inputs.  The scipy figure is a stand-in for the reference's SimpleITK pass
(metrics.py:156-309), which is not what was timed.  The first class's twelve result integers are checked against the
restatement before anything is timed (every class's, unless --no-host).

    python tools/surface_bench.py [--rounds 20] [--warmup 3] [--no-host]

The inputs and the restatement come from tests/surface_ref.py (scipy), the helper of the test suite: the tool runs from
a checkout of the repository, not from an installed package.

A per-kernel split needs a profiler run of its own (rocprofv3 --kernel-trace --stats -- python tools/surface_bench.py
--no-host).  One JSON line on stdout."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "h-denseformer_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np
import torch

import surface_ref as sr
from hdf_rt._lib import check, lib, ptr, stream_ptr

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--no-host", action="store_true", help="skip the scipy timing")
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("surface_bench: no GPU (there is nothing to measure without one)")
dev = torch.device("cuda", 0)
N_CLS = 3


def med(v):
    return sorted(v)[len(v) // 2]


out = {"rounds": a.rounds, "warmup": a.warmup, "volumes": {}}
for shape in ((144, 144, 144), (240, 240, 155)):
    t, p = sr.label_maps(shape, 11, N_CLS)
    td, pd = torch.from_numpy(t).to(dev), torch.from_numpy(p).to(dev)
    ws = torch.empty(lib().hdf_surface_workspace_bytes(*shape), dtype=torch.uint8, device=dev)
    rows = torch.zeros((N_CLS, 12), dtype=torch.int64, device=dev)

    def run(k):
        check(lib().hdf_surface_distances(ptr(td), ptr(pd), k, *shape, ptr(ws), ws.numel(), ptr(rows[k - 1]), None, 0,
                                          stream_ptr()), "hdf_surface_distances")

    for _ in range(a.warmup):
        for k in range(1, N_CLS + 1):
            run(k)
    torch.cuda.synchronize()
    # the restatement on the same inputs: the check of what is about to be timed, and the host figure
    host_s = []
    for k in range(1, N_CLS + 1 if not a.no_host else 2):
        t0 = time.perf_counter()
        ref = sr.surface(t, p, k)["result"]
        host_s.append(time.perf_counter() - t0)
        assert rows[k - 1].cpu().tolist() == ref, (k, rows[k - 1].cpu().tolist(), ref)
    ev = {k: [] for k in range(1, N_CLS + 1)}
    for _ in range(a.rounds):
        for k in ev:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(k)
            e1.record()
            ev[k].append((e0, e1))
    torch.cuda.synchronize()
    per = {k: [e0.elapsed_time(e1) for e0, e1 in v] for k, v in ev.items()}
    res = rows.cpu().tolist()
    row = {"voxels": int(np.prod(shape)), "workspace_MB": round(ws.numel() / 1e6, 1),
           "device_ms_per_class": {str(k): {"median": round(med(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
                                   for k, v in per.items()},
           "device_ms_per_class_median_over_classes": round(med([med(v) for v in per.values()]), 3),
           "class_voxels_T": [r[0] for r in res], "surface_voxels_n": [r[6] for r in res],
           "scipy_restatement_s_per_class": None if a.no_host else [round(s, 3) for s in host_s]}
    out["volumes"]["x".join(map(str, shape))] = row
    print(shape, row, file=sys.stderr)
print(json.dumps(out))
