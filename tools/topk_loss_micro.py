"""Device time of TopKLoss forward + backward (hdf_loss_topk_*) at the benchmarked 3-D geometry (2 x 4 x 128^3) and the 2-D
PI-CAI shape (24 x 2 x 384^2), fp32 and bf16 logits, both forms (the K-vector and reduction='topk'), next to two yardsticks
taken in the same process:

  (a) fused      hdf_loss_topk_forward + hdf_loss_topk_backward through the C ABI on a preallocated workspace
  (b) ce floor   the existing fused cross-entropy (hdf_loss_terms_* with weights 1, 0, one scale) at the same shape: one read
                 of the logits and one write of dlogits, no selection
  (c) torch      the reference's own op sequence in torch on the same GPU: permute, cross_entropy(reduction='none'), topk,
                 mean (or the vector), backward

    python tools/topk_loss_micro.py [--iters 200] [--out profiles/topk_loss_micro.json]

Every leg is warmed up at every shape; the legs alternate inside one loop and each call is timed with its own pair of HIP
events; the median and the spread (min, 10th / 90th percentile) are reported.  Algorithmic bytes of (a): the logits read once,
res written (4 B a voxel), rank written and read back (4 B each), dlogits written; the achieved bytes per second is that
over the median.  One JSON document on stdout and in --out."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "h-denseformer_amd")):
    sys.path.insert(0, p)
import torch  # noqa: E402
from hdf_rt._lib import BF16, F32, check, lib, ptr, stream_ptr  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--k", type=float, default=10)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topk_loss_micro.json"))
a = ap.parse_args()
dev = torch.device("cuda", 0)
SHAPES = {"3d_2x4x128^3": (2, 4, (128, 128, 128)), "2d_picai_24x2x384^2": (24, 2, (384, 384))}
DT = {"fp32": (F32, torch.float32), "bf16": (BF16, torch.bfloat16)}


def med(v):
    return sorted(v)[len(v) // 2]


def pct(v, q):
    return sorted(v)[min(len(v) - 1, int(q * len(v)))]


def legs(b, c, sp, code, tdt, mean):
    d, h, w = ((1,) + sp) if len(sp) == 2 else sp
    n = b * d * h * w
    K = int(n * a.k / 100)
    gen = torch.Generator().manual_seed(3)
    lab = torch.randint(0, c, (b,) + sp, generator=gen)
    onehot = torch.nn.functional.one_hot(lab, c).movedim(-1, 1).float().contiguous().to(dev)
    labd = lab.to(dev)
    x = (torch.randn((b, c) + sp, generator=gen) * 2.0).to(dev).to(tdt).contiguous()
    dl = torch.empty_like(x)
    nbytes = lib().hdf_loss_topk_workspace_bytes(b, d, h, w)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out = torch.empty(1 if mean else K, dtype=torch.float32, device=dev)
    g = torch.ones(1, device=dev) if mean else torch.rand(K, device=dev)
    geom = (code, ptr(x), ptr(onehot), b, c, d, h, w, 0, None, -100, K)
    ws_ce = torch.empty(lib().hdf_loss_workspace_bytes(b), dtype=torch.uint8, device=dev)
    loss_ce, g1 = torch.empty(1, device=dev), torch.ones(1, device=dev)

    def fused():
        check(lib().hdf_loss_topk_forward(*geom, ptr(ws), nbytes, None if mean else ptr(out), ptr(out) if mean else None,
                                          stream_ptr()), "topk forward")
        check(lib().hdf_loss_topk_backward(*geom, ptr(ws), nbytes, None if mean else ptr(g), ptr(g) if mean else None,
                                           ptr(dl), stream_ptr()), "topk backward")

    def ce_floor():
        check(lib().hdf_loss_terms_forward(code, ptr(x), None, None, None, 1, ptr(onehot), b, c, d, h, w, 1.0, 0.0,
                                           ptr(ws_ce), ptr(loss_ce), stream_ptr()), "ce forward")
        check(lib().hdf_loss_terms_backward(code, ptr(x), None, None, None, 1, ptr(onehot), b, c, d, h, w, 1.0, 0.0,
                                            ptr(ws_ce), ptr(g1), ptr(dl), None, None, None, stream_ptr()), "ce backward")

    xt = x.clone().requires_grad_(True)

    def torch_ops():
        xt.grad = None
        perm = (0, 2, 3, 4, 1) if len(sp) == 3 else (0, 2, 3, 1)
        res = torch.nn.functional.cross_entropy(xt.permute(*perm).contiguous().view(-1, c), labd.view(-1), reduction="none")
        vals, _ = torch.topk(res.view(-1), K, sorted=False)
        if mean:
            vals.mean().backward()
        else:
            vals.backward(g.to(vals.dtype))

    esz = x.element_size()
    alg = n * c * esz + 4 * n + 4 * n + 4 * n + n * c * esz
    return dict(fused=fused, ce_floor=ce_floor, torch=torch_ops), n, K, alg


result = {"iters": a.iters, "k_percent": a.k, "device": torch.cuda.get_device_name(0), "rows": []}
for sname, (b, c, sp) in SHAPES.items():
    for dname, (code, tdt) in DT.items():
        for mean in (False, True):
            fns, n, K, alg = legs(b, c, sp, code, tdt, mean)
            for f in fns.values():
                for _ in range(5):
                    f()
            torch.cuda.synchronize()
            ev = {k: [] for k in fns}
            for _ in range(a.iters):
                for k, f in fns.items():            # the legs alternate inside one loop
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    f()
                    e1.record()
                    ev[k].append((e0, e1))
            torch.cuda.synchronize()
            row = {"shape": sname, "dtype": dname, "form": "topk" if mean else "vector", "voxels": n, "K": K,
                   "algorithmic_bytes": alg, "legs": {}}
            for k, pairs in ev.items():
                us = [e0.elapsed_time(e1) * 1e3 for e0, e1 in pairs]
                row["legs"][k] = {"median_us": round(med(us), 1), "min_us": round(min(us), 1), "p10_us": round(pct(us, 0.1), 1),
                                  "p90_us": round(pct(us, 0.9), 1)}
            m = row["legs"]["fused"]["median_us"]
            row["fused_TB_per_s"] = round(alg / m / 1e6, 3)
            row["fused_over_ce_floor"] = round(m / row["legs"]["ce_floor"]["median_us"], 2)
            row["torch_over_fused"] = round(row["legs"]["torch"]["median_us"] / m, 2)
            result["rows"].append(row)
            print("%-22s %-5s %-6s fused %8.1f us (%.3f TB/s)  ce floor %8.1f us  torch %8.1f us" % (
                sname, dname, row["form"], m, row["fused_TB_per_s"], row["legs"]["ce_floor"]["median_us"],
                row["legs"]["torch"]["median_us"]), file=sys.stderr)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as fh:
    json.dump(result, fh, indent=1)
print(json.dumps(result))
