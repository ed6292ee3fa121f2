"""Device time per class of hdf_surface_distances (mask flags, two exact squared distance transforms, gather, select) on
the volumes a user scores -- 128^3, 144^3 and 240x240x155 -- with seeded three-label maps resident on the device, HIP events
around each call after a warm-up; beside it the host time of the scipy restatement of the same definitions
(tests/surface_ref.py) on the same inputs.  The scipy figure is a stand-in for the reference's SimpleITK pass
(metrics.py:156-309), which is not what was timed.  The first class's twelve result integers are checked against the
restatement before anything is timed (every class's, unless --no-host).

Beside each class's hdf_surface_distances call, in the same rounds and alternating with it, the hdf_surface_asd call of
that class (edge flags, two distance transforms seeded from the edge sets, a two-histogram gather, the fp64 sums) and
the host time of its restatement (tests/asd_ref.py: the stand-in for the reference's MONAI pass, utils.py:165-191).  Its
counts are checked exactly and its sums to 1e-12 before anything is timed.

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

import asd_ref as ar
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
for shape in ((128, 128, 128), (144, 144, 144), (240, 240, 155)):
    t, p = sr.label_maps(shape, 11, N_CLS)
    td, pd = torch.from_numpy(t).to(dev), torch.from_numpy(p).to(dev)
    ws = torch.empty(lib().hdf_surface_workspace_bytes(*shape), dtype=torch.uint8, device=dev)
    rows = torch.zeros((N_CLS, 12), dtype=torch.int64, device=dev)
    ws_asd = torch.empty(lib().hdf_surface_asd_workspace_bytes(*shape), dtype=torch.uint8, device=dev)
    rows_asd = torch.zeros((N_CLS, 4), dtype=torch.int64, device=dev)

    def run(k):
        check(lib().hdf_surface_distances(ptr(td), ptr(pd), k, *shape, ptr(ws), ws.numel(), ptr(rows[k - 1]), None, 0,
                                          stream_ptr()), "hdf_surface_distances")

    def run_asd(k):
        check(lib().hdf_surface_asd(ptr(td), ptr(pd), k, *shape, ptr(ws_asd), ws_asd.numel(), ptr(rows_asd[k - 1]), None,
                                    0, stream_ptr()), "hdf_surface_asd")

    for _ in range(a.warmup):
        for k in range(1, N_CLS + 1):
            run(k)
            run_asd(k)
    torch.cuda.synchronize()
    # the restatement on the same inputs: the check of what is about to be timed, and the host figure
    host_s, host_asd_s = [], []
    for k in range(1, N_CLS + 1 if not a.no_host else 2):
        t0 = time.perf_counter()
        ref = sr.surface(t, p, k)["result"]
        host_s.append(time.perf_counter() - t0)
        assert rows[k - 1].cpu().tolist() == ref, (k, rows[k - 1].cpu().tolist(), ref)
        t0 = time.perf_counter()
        ref = ar.asd(t, p, k)
        host_asd_s.append(time.perf_counter() - t0)
        got = rows_asd[k - 1].cpu()
        sums = got[2:].view(torch.float64).tolist()
        assert got[:2].tolist() == ref["counts"], (k, got.tolist(), ref["counts"])
        assert all(abs(g - w) <= 1e-12 * w for g, w in zip(sums, (ref["sumA"], ref["sumB"]))), (k, sums, ref["sumA"], ref["sumB"])
    ev = {k: [] for k in range(1, N_CLS + 1)}
    ev_asd = {k: [] for k in range(1, N_CLS + 1)}
    for _ in range(a.rounds):
        for k in ev:
            for fn, dst in ((run, ev), (run_asd, ev_asd)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn(k)
                e1.record()
                dst[k].append((e0, e1))
    torch.cuda.synchronize()
    per = {k: [e0.elapsed_time(e1) for e0, e1 in v] for k, v in ev.items()}
    per_asd = {k: [e0.elapsed_time(e1) for e0, e1 in v] for k, v in ev_asd.items()}
    res = rows.cpu().tolist()
    row = {"voxels": int(np.prod(shape)), "workspace_MB": round(ws.numel() / 1e6, 1),
           "device_ms_per_class": {str(k): {"median": round(med(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
                                   for k, v in per.items()},
           "device_ms_per_class_median_over_classes": round(med([med(v) for v in per.values()]), 3),
           "class_voxels_T": [r[0] for r in res], "surface_voxels_n": [r[6] for r in res],
           "scipy_restatement_s_per_class": None if a.no_host else [round(s, 3) for s in host_s],
           "asd_workspace_MB": round(ws_asd.numel() / 1e6, 1),
           "asd_device_ms_per_class": {str(k): {"median": round(med(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
                                       for k, v in per_asd.items()},
           "asd_edge_voxels_T_P": [r[:2] for r in rows_asd.cpu().tolist()],
           "asd_restatement_s_per_class": None if a.no_host else [round(s, 3) for s in host_asd_s]}
    out["volumes"]["x".join(map(str, shape))] = row
    print(shape, row, file=sys.stderr)
print(json.dumps(out))
