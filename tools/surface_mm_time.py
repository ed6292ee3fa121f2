"""One hdf_surface_distances_mm call beside one hdf_surface_distances call on the same inputs (HIP-event medians, inputs and
workspaces resident on the device, the two calls alternating), and the two transforms alone, which is where the time goes.

  python tools/surface_mm_time.py [D H W]          (default 128 128 128, the "blobs" masks of tests/surface_ref.py)

One JSON object on the last line."""
import ctypes as C
import json
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "h-denseformer_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np
import torch

import surface_ref as sr
from hdf_rt._lib import check, lib, ptr

DEV = torch.device("cuda", 0)


def st():
    return torch.cuda.current_stream().cuda_stream


def medians(fns, reps=15, warm=2, inner=50):
    """median milliseconds of one call of each callable: `inner` calls between two events (a call is well below a
    millisecond), the callables taking turns inside every repetition"""
    for _ in range(warm):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ts[k].append(e0.elapsed_time(e1) / inner)
    return {k: round(sorted(v)[len(v) // 2], 4) for k, v in ts.items()}


def main():
    shape = tuple(int(a) for a in sys.argv[1:4]) if len(sys.argv) >= 4 else (128, 128, 128)
    v = int(np.prod(shape))
    t, p = sr.blobs(shape, 17 + sum(shape), 0.12, label=3)
    td, pd = torch.from_numpy(t).to(DEV), torch.from_numpy(p).to(DEV)
    L = lib()
    n_int, n_mm = L.hdf_surface_workspace_bytes(*shape), L.hdf_surface_mm_workspace_bytes(*shape)
    ws_int = torch.empty(n_int, dtype=torch.uint8, device=DEV)
    ws_mm = torch.empty(n_mm, dtype=torch.uint8, device=DEV)
    res = torch.zeros(12, dtype=torch.int64, device=DEV)
    flags = torch.zeros(v, dtype=torch.uint8, device=DEV)
    counts = torch.zeros(5, dtype=torch.int64, device=DEV)
    check(L.hdf_op_mask_flags(ptr(td), ptr(pd), 3, *shape, ptr(flags), ptr(counts), st()), "hdf_op_mask_flags")
    d2i = torch.empty(v, dtype=torch.int32, device=DEV)
    d2f = torch.empty(v, dtype=torch.float64, device=DEV)
    aniso, unit = (C.c_double * 3)(3.0, 0.5, 0.5), (C.c_double * 3)(1.0, 1.0, 1.0)

    def mm(sp):
        return lambda: check(L.hdf_surface_distances_mm(ptr(td), ptr(pd), 3, *shape, sp, ptr(ws_mm), n_mm, ptr(res), st()),
                             "hdf_surface_distances_mm")

    fns = {
        "surface_distances_ms": lambda: check(L.hdf_surface_distances(ptr(td), ptr(pd), 3, *shape, ptr(ws_int), n_int,
                                                                       ptr(res), None, 0, st()), "hdf_surface_distances"),
        "surface_distances_mm_3_05_05_ms": mm(aniso),
        "surface_distances_mm_unit_ms": mm(unit),
        "edt_sq_ms": lambda: check(L.hdf_op_edt_sq(ptr(flags), 4, *shape, ptr(d2i), ptr(ws_int), n_int, st()), "hdf_op_edt_sq"),
        "edt_sq_mm_3_05_05_ms": lambda: check(L.hdf_op_edt_sq_mm(ptr(flags), 4, *shape, aniso, ptr(d2f), ptr(ws_mm), n_mm,
                                                                 st()), "hdf_op_edt_sq_mm"),
    }
    out = medians(fns)
    out.update(shape=list(shape), masks="blobs", workspace_bytes=n_int, workspace_mm_bytes=n_mm,
               device=torch.cuda.get_device_name(0))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
