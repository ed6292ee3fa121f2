"""Generate tests/golden/g12_topk_loss.npz by running the REAL reference's TopKLoss (loss/cross_entropy.py:26-43).

TEST INFRASTRUCTURE, CPU only: the reference is imported at generation time (oracle.make_goldens._import_reference) and is
not needed afterwards; the output is pure data.  Usage:   python tools/make_topk_goldens.py

For four small cases of tests/topk_ref.py (GOLDEN_CASES: the three smallest and `ignore0`, the one with ignore_index and
class weights; inputs from the case's seed) the file holds the fp32 logits,
the class map (uint8), K and the reference's K-vector SORTED DESCENDING -- torch.topk(sorted=False) leaves its order
unspecified.  The reference is built as TopKLoss(weight, ignore_index, k, reduction='mean'): the vector comes back all the
same (its constructor's reduce=False makes the 'mean' branch dead code), which tests/test_topk_ref_cpu.py asserts."""
import json
import os
import sys

sys.dont_write_bytecode = True          # the reference mount must stay untouched
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "h-denseformer_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import topk_ref as tr  # noqa: E402
from oracle import make_goldens as mg  # noqa: E402


def main():
    torch.manual_seed(0)
    mg._import_reference()
    from loss.cross_entropy import TopKLoss
    rec = dict(cases=np.array(json.dumps({k: [list(tr.CASES[k][0])] + list(tr.CASES[k][1:]) for k in tr.GOLDEN_CASES})),
               torch_version=np.array(torch.__version__))
    for case in tr.GOLDEN_CASES:
        x, lab = tr.base_inputs(case)
        c, k = tr.CASES[case][2], tr.CASES[case][3]
        onehot = torch.nn.functional.one_hot(lab, c).movedim(-1, 1).float()
        w = tr.case_weight(case, torch.float32)
        vec = TopKLoss(weight=w, ignore_index=tr.case_ignore(case), k=k, reduction="mean")(x, onehot)
        assert vec.dim() == 1, "the reference returned a reduced value"
        rec[case + "_logits"] = x.numpy()
        rec[case + "_labels"] = lab.numpy().astype(np.uint8)
        rec[case + "_K"] = np.int64(vec.numel())
        rec[case + "_topk_desc"] = np.sort(vec.detach().numpy())[::-1].copy()
        print("g12", case, "K", vec.numel(), "max", float(vec.max()), "min", float(vec.min()))
    np.savez_compressed(os.path.join(mg.OUT, "g12_topk_loss.npz"), **rec)


if __name__ == "__main__":
    main()
