"""Generate the two-class loss fixtures tests/golden/g11_focal_loss.npz and g11_focal_2d_train.npz by running the REAL
reference's FocalLoss / FLPlusDice / DeepSuperloss (loss/cross_entropy.py:45-73, loss/combine_loss.py:37-79).

TEST INFRASTRUCTURE, CPU only: the reference is imported at generation time (oracle.make_goldens._import_reference) and
is not needed afterwards; the outputs are pure data.  Usage:   python tools/make_focal_goldens.py

  g11_focal_loss      loss + dL/dlogits of every scale for the cases in CASES (the case table is stored in the file as
                      JSON under "cases"): DeepSuperloss(FocalLoss('sum')) on 3-D C=2 / C=4 and 2-D C=2 logits (4
                      scales, widths 24/12/6/3), stand-alone FocalLoss settings, FLPlusDice with and without class weights
                      and ignore_index, soft targets, and the saturated voxels of the issue's table in both directions.
  g11_focal_2d_train  HDenseFormer_2D(3, 2, 16, (64, 96), td=8), B=2, hash dropout on, DeepSuperloss(FocalLoss('sum')),
                      one Adam step of the reference's _get_optimizer: the record format of g6_2d_train.
"""
import json
import os
import sys

sys.dont_write_bytecode = True          # the reference mount must stay untouched
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle import make_goldens as mg  # noqa: E402

OUT = mg.OUT
SAT_GAPS = (5.0, 20.0, 28.0, 40.0, 200.0, -40.0)

# name: geometry (C, spatial of scale 0, scales, target kind) and criterion (kind, settings).  kind "focal":
# FocalLoss(alpha, gamma, reduction=red); "flpd": FLPlusDice(weight, ignore_index); deep: wrapped in DeepSuperloss.
CASES = {
    "deep3_c2": dict(c=2, sp=(8, 16, 16), n=4, tgt="onehot", kind="focal", deep=True, alpha=1, gamma=2, red="sum"),
    "deep3_c4": dict(c=4, sp=(8, 16, 24), n=4, tgt="onehot", kind="focal", deep=True, alpha=1, gamma=2, red="sum"),
    "deep2_c2": dict(c=2, sp=(40, 24), n=4, tgt="onehot", kind="focal", deep=True, alpha=1, gamma=2, red="sum"),
    "mean_c2": dict(c=2, sp=(8, 16, 12), n=1, tgt="onehot", kind="focal", deep=False, alpha=1, gamma=2, red="mean"),
    "a025_g0": dict(c=2, sp=(8, 16, 12), n=1, tgt="onehot", kind="focal", deep=False, alpha=0.25, gamma=0, red="sum"),
    "am1_g3": dict(c=3, sp=(8, 16, 12), n=1, tgt="onehot", kind="focal", deep=False, alpha=-1, gamma=3, red="sum"),
    "soft_c3": dict(c=3, sp=(8, 16, 12), n=1, tgt="soft", kind="focal", deep=False, alpha=0.25, gamma=2, red="sum"),
    "deep_flpd": dict(c=3, sp=(8, 16, 16), n=4, tgt="onehot", kind="flpd", deep=True, weight=None, ignore=0),
    "flpd_w": dict(c=4, sp=(8, 16, 12), n=1, tgt="onehot", kind="flpd", deep=False, weight=[0.2, 1.0, 2.5, 0.6],
                   ignore=0),
    "flpd_all": dict(c=2, sp=(8, 16, 12), n=1, tgt="onehot", kind="flpd", deep=False, weight=None, ignore=None),
    # one row of 2 x 6 voxels, target class 1; logits (gap, 0) and (0, gap): the target's margin is -gap and +gap
    "sat": dict(c=2, sp=(2, len(SAT_GAPS)), n=1, tgt="onehot", kind="focal", deep=False, alpha=1, gamma=2, red="sum"),
}


def _criterion(ref_loss, case):
    FocalLoss, FLPlusDice, DeepSuperloss = ref_loss
    if case["kind"] == "focal":
        crit = FocalLoss(alpha=case["alpha"], gamma=case["gamma"], reduction=case["red"])
    else:
        w = None if case["weight"] is None else torch.tensor(case["weight"])
        crit = FLPlusDice(weight=w, ignore_index=case["ignore"])
    return DeepSuperloss(criterion=crit) if case["deep"] else crit


def _inputs(tag, case, seed):
    g = torch.Generator().manual_seed(seed)
    c, sp = case["c"], case["sp"]
    if tag == "sat":
        gaps = torch.tensor(SAT_GAPS)
        z = torch.zeros(1, 2, 2, len(SAT_GAPS))
        z[0, 0, 0], z[0, 1, 1] = gaps, gaps            # row 0: the other class leads by gap; row 1: the target does
        t = torch.zeros(1, 2, 2, len(SAT_GAPS))
        t[:, 1] = 1.0
        return [z], t
    if case["tgt"] == "soft":
        t = torch.rand((2, c) + sp, generator=g)
    else:
        lab = torch.randint(0, c, (2,) + sp, generator=g)
        t = torch.nn.functional.one_hot(lab, c).movedim(-1, 1).float()
    outs = [torch.randn((2, c) + tuple(s >> i for s in sp), generator=g) * 2.0 for i in range(case["n"])]
    return outs, t


def golden_focal_loss(ref_loss):
    rec = dict(cases=np.array(json.dumps(CASES)), torch_version=torch.__version__)
    for k, (tag, case) in enumerate(CASES.items()):
        outs, t = _inputs(tag, case, 100 + k)
        crit = _criterion(ref_loss, case)
        outs = [o.clone().requires_grad_(True) for o in outs]
        loss = crit(outs, t) if case["deep"] else crit(outs[0], t)
        loss.backward()
        rec[tag + "_loss"] = loss.item()
        rec[tag + "_target"] = t.numpy().astype(np.uint8) if case["tgt"] == "onehot" else t.numpy()
        for i, o in enumerate(outs):
            rec[f"{tag}_logits{i}"] = o.detach().numpy()
            rec[f"{tag}_grad{i}"] = o.grad.numpy()
        print("g11", tag, loss.item())
    np.savez_compressed(os.path.join(OUT, "g11_focal_loss.npz"), **rec)


def main():
    torch.manual_seed(0)
    ref = mg._import_reference()
    from loss.combine_loss import FLPlusDice
    from loss.cross_entropy import FocalLoss
    golden_focal_loss((FocalLoss, FLPlusDice, ref["DeepSuperloss"]))
    # golden_model builds DeepSuperloss(criterion=ref["CEPlusDice"](weight=None, ignore_index=0)): hand it the focal loss
    # the trainer builds for two-class runs (trainer.py:755-757) instead
    ref_focal = dict(ref, CEPlusDice=lambda weight=None, ignore_index=None: FocalLoss(reduction="sum"))
    mg.golden_model(ref_focal, "g11_focal_2d_train", (3, 2, 16, (64, 96), 8), 2, 1606, sample_step=2, inter_step=4,
                    n_samples=16, adam_step=True, full_grads=("conv1x1.weight", "upconv_2.bias",
                                                              "block_2_1_left.conv.weight",
                                                              "attns.1.patch_embeddings.weight"))


if __name__ == "__main__":
    main()
