"""Drop-in `loss.combine_loss` (reference loss/combine_loss.py:8-79) backed by the fused HIP loss.

Supported: what trainer.py:743-771 (_get_loss) builds for the H-DenseFormer runs --
DeepSuperloss(criterion=CEPlusDice(weight=class_weight or None, ignore_index=0)) and, for two-class runs,
DeepSuperloss(criterion=FocalLoss(reduction='sum')) -- plus FLPlusDice(weight, ignore_index) and ignore_index=None,
with the BinaryDiceLoss defaults (smooth 1e-5, p 1, reduction 'mean'), and DeepSuperloss(criterion=TopKLoss(...,
reduction='topk')) = sum_i 2^-i * (mean of the K_i largest per-voxel losses of scale i), K_i from that scale's voxel count,
the target read at index << i (F.interpolate(nearest) by exactly 2^i) without a down-sampled copy.  A TopKLoss in the
reference's vector form raises here as it does in the reference (four vectors of different lengths cannot be summed).
Anything else raises: there is no eager fallback."""
from torch import nn

from hdf_rt.loss_fn import DeepSuperCEDice, DeepSuperFocalDice, TopKVoxelCE

from .cross_entropy import FocalLoss, TopKLoss

_DICE_DEFAULTS = dict(smooth=1e-5, p=1, reduction="mean")


def check_dice_kwargs(kwargs):
    """BinaryDiceLoss keyword arguments (dice_loss.py:20-25): the kernels implement the defaults (trainer.py:761 passes
    p=1 explicitly); k only matters for reduction='topk'."""
    for k, v in kwargs.items():
        if k == "k":
            continue
        if k not in _DICE_DEFAULTS or v != _DICE_DEFAULTS[k]:
            raise NotImplementedError(f"fused Dice loss implements BinaryDiceLoss(smooth=1e-5, p=1, reduction='mean'); "
                                      f"got {k}={v!r}")


class CEPlusDice(nn.Module):
    def __init__(self, weight=None, ignore_index=None, **kwargs):
        super().__init__()
        self.weight, self.ignore_index, self.kwargs = weight, ignore_index, kwargs

    def _check(self):
        check_dice_kwargs(self.kwargs)

    def _spec(self, target):
        return (target, 1.0, 1.0, self.weight, self.ignore_index)

    def forward(self, predict, target):
        assert predict.size() == target.size()
        self._check()
        return DeepSuperCEDice.apply(self._spec(target), predict)


class FLPlusDice(nn.Module):
    """DiceLoss(weight, ignore_index, **kwargs) + FocalLoss(reduction='mean') in one pass; the class weight applies to
    the Dice term only."""

    def __init__(self, weight=None, ignore_index=None, **kwargs):
        super().__init__()
        check_dice_kwargs(kwargs)
        self.weight, self.ignore_index, self.kwargs = weight, ignore_index, kwargs

    def _check(self):
        check_dice_kwargs(self.kwargs)

    def _spec(self, target):
        return (target, 1.0, 1, 2, "mean", 1.0, self.weight, self.ignore_index)

    def forward(self, predict, target):
        assert predict.size() == target.size()
        self._check()
        return DeepSuperFocalDice.apply(self._spec(target), predict)


class DeepSuperloss(nn.Module):
    def __init__(self, criterion=None):
        super().__init__()
        self.loss = criterion

    def forward(self, input, target):
        if isinstance(self.loss, TopKLoss):
            if self.loss.reduction != "topk":
                raise NotImplementedError("DeepSuperloss(TopKLoss): the reference's vector form cannot be summed over "
                                          "scales (the reference raises too); build TopKLoss(..., reduction='topk')")
            outs = list(input)                 # (the settings were checked when the criterion was built)
            if not 1 <= len(outs) <= 4:
                raise NotImplementedError("fused DeepSuperloss handles 1..4 deep-supervision scales")
            total = TopKVoxelCE.apply(self.loss._spec(target, 0), outs[0])
            for i, out in enumerate(outs[1:], 1):
                total = total + TopKVoxelCE.apply(self.loss._spec(target, i), out) * (1.0 / (1 << i))
            return total
        if isinstance(self.loss, CEPlusDice):
            node = DeepSuperCEDice
        elif isinstance(self.loss, (FLPlusDice, FocalLoss)):
            node = DeepSuperFocalDice
        else:
            raise NotImplementedError("fused DeepSuperloss needs criterion=CEPlusDice(...), FLPlusDice(...), "
                                      "FocalLoss(...) or TopKLoss(..., reduction='topk')")
        self.loss._check()
        return node.apply(self.loss._spec(target), *list(input))
