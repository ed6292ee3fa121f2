"""Drop-in `loss.cross_entropy` (reference loss/cross_entropy.py).

CrossentropyLoss (:8-22): mean cross-entropy of the logits against argmax(one-hot target), optionally class-weighted like
torch.nn.CrossEntropyLoss(weight=..), on the fused HIP loss kernels (the Dice term weighted 0) -- no permuted copy of the
logits.  FocalLoss (:45-73, the loss trainer.py:755-757 builds for two-class runs): the focal term of the fused kernels
(hdf_loss_focal_*), reductions 'sum' and 'mean', gamma 0 or >= 1; other settings raise when the module is built.
TopKLoss (:26-43, the loss trainer.py:751-753 builds for loss_fun='TopKLoss'): per-voxel weighted cross-entropy and an exact
top-K select on the device (hdf_loss_topk_*).  16-bit logits are evaluated in fp32 from storage (the reference raises on
them with an fp32 target).  FLLoss is not provided (nothing in the reference builds it).  There is no eager fallback."""
from torch import nn

from hdf_rt.loss_fn import DeepSuperCEDice, DeepSuperFocalDice, TopKVoxelCE, focal_settings, topk_settings


class CrossentropyLoss(nn.Module):
    def __init__(self, weight=None, **kwargs):
        super().__init__()
        if kwargs:
            raise NotImplementedError(f"fused CrossentropyLoss implements weight= only (got {sorted(kwargs)})")
        self.weight = weight

    def forward(self, inp, target):
        return DeepSuperCEDice.apply((target, 1.0, 0.0, self.weight, 0), inp)


class TopKLoss(nn.Module):
    """The K = int(num_voxels * k / 100) largest per-voxel cross-entropy values res[v] = weight[t_v] * nll_v (0 where t_v ==
    ignore_index), t the arg-max of the one-hot target.

    reduction None, 'mean' and 'sum' all behave as the reference does: its constructor passes reduce=False to
    torch.nn.CrossEntropyLoss, which overwrites self.reduction with 'none', so the 'mean' / 'sum' branches of its forward
    are dead and the result is the K-vector of torch.topk(..., sorted=False).  The reference leaves the vector's order open;
    here it is ascending voxel index (b, d, h, w).  It is differentiable with respect to the logits for an upstream
    gradient vector g[K]; as in the reference, backward() on it needs that vector, and DeepSuperloss cannot sum it over
    scales -- the reference cannot train with TopKLoss as trainer.py:751-753 builds it.

    reduction='topk' (the one extension, named after BinaryDiceLoss's reduction, loss/dice_loss.py:44-46) returns the fp32
    scalar mean of those K values: the form a trainer can use, alone or in DeepSuperloss.

    A value equal to the K-th largest is taken lowest voxel index first; a NaN per-voxel loss counts as the largest, as in
    torch.topk.  K == 0 gives an empty vector, and raises ValueError for 'topk' (the mean of nothing).  A negative class
    weight raises ValueError."""

    def __init__(self, weight=None, ignore_index=-100, k=10, reduction=None):
        super().__init__()
        topk_settings(weight, ignore_index, k, reduction)      # once, here: reading a device weight synchronises
        self.weight, self.ignore_index, self.k, self.reduction = weight, ignore_index, k, reduction

    def _spec(self, target, scale_shift=0):
        return (target, self.weight, self.ignore_index, self.k, self.reduction == "topk", scale_shift)

    def forward(self, inp, target):
        return TopKVoxelCE.apply(self._spec(target), inp)


class FocalLoss(nn.Module):
    """Focal loss function for binary segmentation (num_classes is unused, as in the reference)."""

    def __init__(self, alpha=1, gamma=2, num_classes=2, reduction="sum"):
        super().__init__()
        focal_settings(alpha, gamma, reduction)
        self.alpha = alpha
        self.gamma = gamma
        self.num_classes = num_classes
        self.reduction = reduction

    def _check(self):
        focal_settings(self.alpha, self.gamma, self.reduction)

    def _spec(self, target):
        return (target, 1.0, self.alpha, self.gamma, self.reduction, 0.0, None, 0)

    def forward(self, inputs, targets):
        return DeepSuperFocalDice.apply(self._spec(targets), inputs)
