"""Drop-in `loss.cross_entropy` (reference loss/cross_entropy.py).

CrossentropyLoss (:8-22): mean cross-entropy of the logits against argmax(one-hot target), optionally class-weighted like
torch.nn.CrossEntropyLoss(weight=..), on the fused HIP loss kernels (the Dice term weighted 0) -- no permuted copy of the
logits.  FocalLoss (:45-73, the loss trainer.py:755-757 builds for two-class runs): the focal term of the fused kernels
(hdf_loss_focal_*), reductions 'sum' and 'mean', gamma 0 or >= 1; other settings raise when the module is built.
16-bit logits are evaluated in fp32 from storage (the reference raises on them with an fp32 target).  TopKLoss and
FLLoss are not provided.  There is no eager fallback."""
from torch import nn

from hdf_rt.loss_fn import DeepSuperCEDice, DeepSuperFocalDice, focal_settings


class CrossentropyLoss(nn.Module):
    def __init__(self, weight=None, **kwargs):
        super().__init__()
        if kwargs:
            raise NotImplementedError(f"fused CrossentropyLoss implements weight= only (got {sorted(kwargs)})")
        self.weight = weight

    def forward(self, inp, target):
        return DeepSuperCEDice.apply((target, 1.0, 0.0, self.weight, 0), inp)


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
