"""What the lesion-wise HD95 costs on crops against the loop it replaces.  One process, one 128^3 volume of about 30 truth
lesions (seeded ellipsoids on a jittered grid; the prediction keeps most of them displaced and resized, misses some and adds
a few of its own), class 1.

  crop path   hdf_rt.lesion_wise_scores(hd95=True): the Dice half, two component tables, ONE hdf_lesion_surface over the
              kept lesions with a non-empty P_j, two copies to the host
  loop        what a user of the parent commit writes for the same numbers: lesion_wise_scores() for the Dice half and
              the lists P_j, the two id maps once more (connected_components; the wrapper does not return them), then per
              kept lesion two FULL-VOLUME masks built with torch on the device and one hdf_rt.surface_scores call

Both are timed with device events around the whole call after warm-up (the calls end in a copy to the host, so the events
bracket the host work too); the median of 20 runs is reported, in voxels and with a spacing.  The per-lesion numbers of the
two paths are compared first and must agree in every bit.  Prints one JSON line.

    python tools/lesion_hd_bench.py [--size 128] [--reps 20] [--seed 0]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "h-denseformer_amd")):
    sys.path.insert(0, p)
import numpy as np
import torch

from hdf_rt import binary_dilation, connected_components, lesion_wise_scores, surface_scores

DEV = torch.device("cuda", 0)
SPACING = (2.5, 0.8, 1.1)


def volume(size, seed):
    """(pred, truth) uint8 [size]^3: one ellipsoid per cell of a 3 x 3 x 4 grid, far enough apart to stay apart when dilated"""
    rng = np.random.default_rng(seed)
    z, y, x = np.ogrid[:size, :size, :size]
    truth, pred = np.zeros((size,) * 3, np.uint8), np.zeros((size,) * 3, np.uint8)

    def ball(c, r):
        return ((z - c[0]) / r[0]) ** 2 + ((y - c[1]) / r[1]) ** 2 + ((x - c[2]) / r[2]) ** 2 <= 1.0

    cells = (3, 3, 4)
    for i in np.ndindex(*cells):
        c = [(k + 0.5) * size / n + rng.uniform(-3, 3) for k, n in zip(i, cells)]
        r = [rng.uniform(3.0, 0.5 * size / n - 8.0) for n in cells]
        truth[ball(c, r)] = 1
        kind = rng.random()
        if kind < 0.15:
            continue                                              # missed
        shift, scale = rng.uniform(-2.0, 2.0, 3), rng.uniform(0.6, 1.3)
        hit = ball([a + b for a, b in zip(c, shift)], [scale * v for v in r])
        if kind > 0.8:                                            # split in two
            hit[..., int(c[2])] = False
        pred[hit] = 1
    for _ in range(3):                                            # spurious, in the corners of cells
        c = [rng.integers(0, n) * size / n + 2 for n in cells]
        pred[ball(c, [2.0, 2.0, 2.0])] = 1
    return pred, truth


def gpu_ms(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return sorted(ts)[len(ts) // 2]


def loop(pred, truth, spacing):
    """{lesion id: (HausdorffDistance, HausdorffDistance95)} by full-volume masks, one surface_scores call a lesion"""
    base = lesion_wise_scores(pred, truth, 1)
    g = (truth == 1).to(torch.uint8)
    ids_t, _ = connected_components(binary_dilation(g, 18, 3), 26, 0)
    ids_p, _ = connected_components(pred, 26, 1)
    out = {}
    for les in base["lesions"]:
        if not les["pred"]:
            continue
        T = ((ids_t == les["id"]) & (g != 0)).to(torch.uint8)
        P = torch.isin(ids_p, torch.tensor(les["pred"], dtype=torch.int32, device=pred.device)).to(torch.uint8)
        s = surface_scores(T, P, [1], spacing)[0]
        out[les["id"]] = (s["HausdorffDistance"], s["HausdorffDistance95"])
    return out


def crop_voxels(pred, truth, scored):
    """the summed voxels of the crops the wrapper carves: the box of the dilated truth lesion and P_j, grown by one voxel"""
    g = (truth == 1).to(torch.uint8)
    ids_t, _ = connected_components(binary_dilation(g, 18, 3), 26, 0)
    ids_p, _ = connected_components(pred, 26, 1)
    total = 0
    for les in scored:
        m = (ids_t == les["id"]) | torch.isin(ids_p, torch.tensor(les["pred"], dtype=torch.int32, device=pred.device))
        idx = torch.nonzero(m)
        lo, hi = idx.min(0).values.tolist(), idx.max(0).values.tolist()
        total += int(np.prod([min(h + 1, s - 1) - max(l - 1, 0) + 1 for l, h, s in zip(lo, hi, m.shape)]))
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    hp, ht = volume(a.size, a.seed)
    pred, truth = torch.from_numpy(hp).to(DEV), torch.from_numpy(ht).to(DEV)
    row = dict(volume=[a.size] * 3, reps=a.reps)
    for name, sp in (("voxels", None), ("mm", SPACING)):
        got = lesion_wise_scores(pred, truth, 1, hd95=True, spacing=sp)
        scored = [les for les in got["lesions"] if les["pred"]]
        want = loop(pred, truth, sp)
        same = all(np.array([les["hd"], les["hd95"]]).tobytes() == np.array(want[les["id"]]).tobytes() for les in scored)
        if not same or len(want) != len(scored):
            raise SystemExit(f"the two paths disagree ({name})")
        if sp is None:
            row.update(truth_lesions=len(got["lesions"]), scored_lesions=len(scored), false_positives=got["fp"],
                       lesion_hd95=got["lesion_hd95"], crop_voxels=crop_voxels(pred, truth, scored),
                       loop_voxels=len(scored) * a.size ** 3)
            row["dice_half_ms"] = gpu_ms(lambda: lesion_wise_scores(pred, truth, 1), a.reps)
        row[f"crop_path_ms_{name}"] = gpu_ms(lambda: lesion_wise_scores(pred, truth, 1, hd95=True, spacing=sp), a.reps)
        row[f"loop_ms_{name}"] = gpu_ms(lambda: loop(pred, truth, sp), a.reps)
    print(json.dumps(row))


if __name__ == "__main__":
    main()
