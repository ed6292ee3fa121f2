"""Host time of `scaler.step(opt)` + `scaler.update()` for FlatAdam with fp16 storage at the benchmark geometry
(HDenseFormer_32, 4x128^3, batch 2): the wall clock the training loop's thread spends inside the two calls, once as the
loop runs them (the device still busy with the backward: a host synchronisation inside them waits for it) and once after
a torch.cuda.synchronize() (the calls' own host work).

    python tools/scaler_host_time.py [--root TREE] [--steps 12]

--root: another checkout of this repository (built) to measure instead of this one, for before / after pairs on one
machine.  One JSON line on stdout."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--steps", type=int, default=12)
a = ap.parse_args()
ROOT = os.path.abspath(a.root)
for p in (ROOT, os.path.join(ROOT, "h-denseformer_amd")):
    sys.path.insert(0, p)
import torch
from hdf_rt.optim import FlatAdam
from loss.combine_loss import CEPlusDice, DeepSuperloss
from models.HDenseFormer import HDenseFormer

dev = torch.device("cuda", 0)
torch.manual_seed(0)
net = HDenseFormer(4, 4, 32, image_size=(128, 128, 128), transformer_depth=24).to(dev)
net.train()
net.compute_dtype = "fp16"
crit = DeepSuperloss(criterion=CEPlusDice(weight=None, ignore_index=0))
opt = FlatAdam(net, lr=1e-3, weight_decay=1e-4)
scaler = torch.amp.GradScaler("cuda", init_scale=256.0)
g = torch.Generator().manual_seed(1)
x = torch.rand(2, 4, 128, 128, 128, generator=g).to(dev)
lab = torch.randint(0, 4, (2, 128, 128, 128), generator=g)
target = torch.nn.functional.one_hot(lab, 4).permute(0, 4, 1, 2, 3).float().contiguous().to(dev)


def step(drain):
    opt.zero_grad()
    loss = crit(net(x), target)
    scaler.scale(loss).backward()
    if drain:
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    scaler.step(opt)
    scaler.update()
    return (time.perf_counter() - t0) * 1e3


for _ in range(4):
    step(False)
torch.cuda.synchronize()
in_loop, drained = [], []
for _ in range(a.steps):
    in_loop.append(step(False))
torch.cuda.synchronize()
for _ in range(a.steps):
    drained.append(step(True))
torch.cuda.synchronize()
med = lambda v: sorted(v)[len(v) // 2]
print(json.dumps({"root": ROOT, "amp_scaling_in_kernel": bool(getattr(opt, "_step_supports_amp_scaling", False)),
                  "scaler_step_update_host_ms": {"in_loop_median": round(med(in_loop), 3),
                                                 "device_idle_median": round(med(drained), 3),
                                                 "in_loop_min": round(min(in_loop), 3),
                                                 "device_idle_min": round(min(drained), 3)},
                  "final_scale": scaler.get_scale()}))
