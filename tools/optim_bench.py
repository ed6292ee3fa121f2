"""Kernel time and achieved HBM bandwidth of the flat optimizer steps (hdf_optim_step: Adam, AdamW, SGD) next to
hdf_adam_step, in one process on the flat buffer of the benchmark geometry (HDenseFormer_32 at 4x128^3: 15.43 M fp32
elements).  The four calls are interleaved round by round and each is timed with its own pair of HIP events; a round is
repeated, so the spread between two measurements of the SAME call in one round is printed next to the differences.

    python tools/optim_bench.py [--rounds 40] [--n ELEMENTS]

Bytes per element: 29 for Adam / AdamW (p, m, v read and written, g and one mask byte read), 21 for SGD.  The event pair
of hdf_optim_step spans its one-thread prologue launch too.  One JSON line on stdout."""
import argparse
import json
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "h-denseformer_amd")):
    sys.path.insert(0, p)
import torch
from hdf_rt._lib import check, lib, ptr, stream_ptr

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=40)
ap.add_argument("--n", type=int, default=0, help="elements (default: the flat buffer of the benchmark geometry)")
a = ap.parse_args()

dev = torch.device("cuda", 0)
n = a.n
if not n:
    from hdf_rt import _lib
    from hdf_rt.runtime import Plan
    n = Plan(4, 4, 32, (128, 128, 128), 24, _lib.F32).param_floats
gen = torch.Generator().manual_seed(0)
p0 = torch.randn(n, generator=gen).to(dev)
g = (torch.randn(n, generator=gen) * 0.01).to(dev)
mask = (torch.rand(n, generator=gen) < 0.9).to(torch.uint8).to(dev)


class Case:
    def __init__(self, name, rule, nbytes):
        self.name, self.rule, self.bytes = name, rule, nbytes
        self.p, self.s1, self.s2 = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
        self.ctl = torch.zeros(8, dtype=torch.int32, device=dev)
        self.step, self.ms = 0, [[], []]

    def run(self):
        self.step += 1
        if self.rule is None:
            check(lib().hdf_adam_step(ptr(self.p), ptr(g), ptr(self.s1), ptr(self.s2), ptr(mask), n, 1e-3, 0.9, 0.999,
                                      1e-8, 1e-4, self.step, 1.0, stream_ptr()), self.name)
        else:
            sgd = self.rule == 2
            check(lib().hdf_optim_step(self.rule, ptr(self.p), ptr(g), ptr(self.s1), None if sgd else ptr(self.s2),
                                       ptr(mask), n, 1e-3, 1e-3, 1e-4, 0.0, 0.9, 0.999, 1e-8, int(sgd), 1.0, None, None,
                                       ptr(self.ctl), stream_ptr()), self.name)

    def timed(self, slot):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        self.run()
        e1.record()
        self.ms[slot].append((e0, e1))


cases = [Case("hdf_adam_step (adam_kernel)", None, 29), Case("hdf_optim_step Adam", 0, 29),
         Case("hdf_optim_step AdamW", 1, 29), Case("hdf_optim_step SGD", 2, 21)]
for c in cases:
    for _ in range(3):
        c.run()
torch.cuda.synchronize()
for _ in range(a.rounds):
    for slot in (0, 1):             # every call twice per round: the second pass gives the same-call spread
        for c in cases:
            c.timed(slot)
torch.cuda.synchronize()


def med(v):
    return sorted(v)[len(v) // 2]


out = {"elements": n, "rounds": a.rounds, "cases": {}}
base = None
for c in cases:
    t = [[e0.elapsed_time(e1) * 1e3 for e0, e1 in s] for s in c.ms]
    both = t[0] + t[1]
    m = med(both)
    row = {"median_us": round(m, 2), "min_us": round(min(both), 2), "TB_per_s": round(c.bytes * n / m / 1e6, 3),
           "bytes_per_element": c.bytes,
           "same_call_pair_diff_us": {"median_abs": round(med([abs(x - y) for x, y in zip(*t)]), 2),
                                      "max_abs": round(max(abs(x - y) for x, y in zip(*t)), 2)}}
    if base is None:
        base = t
    else:
        d = [x - y for x, y in zip(t[0] + t[1], base[0] + base[1])]
        row["minus_adam_kernel_us"] = {"median": round(med(d), 2), "min": round(min(d), 2), "max": round(max(d), 2)}
    out["cases"][c.name] = row
    print(f"{c.name:32s} median {m:8.2f} us  min {min(both):8.2f} us  {row['TB_per_s']:.3f} TB/s", file=sys.stderr)
print(json.dumps(out))
